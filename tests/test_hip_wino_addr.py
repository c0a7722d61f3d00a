"""The Winograd kernels' K loop without address arithmetic (csrc/conv_wino.hip; conv_wino.hpp WinoLoop1): two stages per trip with
the LDS buffer parity a compile-time constant, every LDS address a per-lane register plus an immediate offset, the weights through
one buffer descriptor with the chunk in the scalar offset.  Launches with an odd number of stages per tile keep the one-stage trip.
Only addresses are formed differently, and the input transform's packed operations are written as instructions (pk_sub / pk_fma /
pk_hi_pm_lo) -- every floating-point operation, its operands and its order are what they were -- so:

  1. outputs and fused GroupNorm records equal conv_wino1_kernel's bit for bit (conv_wino1.hip is untouched; tests/test_hip_wino.py
     documents it as bit-identical to WinoCfg<4>) on every combination that kernel serves: plain / two sources / up-sampled input,
     activation on / off, residual none / same / RS_DOWN.  The 64-channel kernel (WinoCfg<2>) and the split kernel of the 16 x 16
     level, which conv_wino1_kernel does not serve, are compared with it through zero-padded output channels (64 -> 128) and on the
     same 16 x 16 shape: a channel's sums never depend on the other channels of the launch.
  2. the SKIP form (folded 1x1 projection, conv_wino1_kernel has none) and the up-sampling form against the fp64 convolution at the
     bar of tests/_tol.py.

Shapes: Cout = 128, 32 x 32 images, B = 3 (two tiles or more per workgroup and the clamped last tile); Cin = 16 (one stage per tile:
odd, the one-stage trip), 32 (one trip per tile), 40 (three stages, the last half full: odd), 64, 128 + 128 from two sources."""
import pytest
import torch

from oracle import fixtures as fx
from tests import _tol

pytestmark = pytest.mark.gpu

RS_NONE, RS_UP, RS_DOWN = 0, 1, 2
# name: (B, Ca, Cb, Cout, H, W, up, act, res); (H, W) is the output size, res in none / same / down
CASES = {
    "cin16": (3, 16, 0, 128, 32, 32, 0, 1, "none"),
    "cin32": (3, 32, 0, 128, 32, 32, 0, 1, "none"),
    "cin40": (3, 40, 0, 128, 32, 32, 0, 1, "none"),
    "cin64": (3, 64, 0, 128, 32, 32, 0, 1, "none"),
    "cin64_same": (3, 64, 0, 128, 32, 32, 0, 1, "same"),
    "cin64_down": (3, 64, 0, 128, 32, 32, 0, 1, "down"),
    "cin64_noact": (3, 64, 0, 128, 32, 32, 0, 0, "none"),
    "cin40_noact": (3, 40, 0, 128, 32, 32, 0, 0, "same"),
    "two_sources": (3, 128, 128, 128, 32, 32, 0, 1, "none"),
    "up": (3, 64, 0, 128, 32, 32, 1, 1, "none"),
    "up_cin40": (3, 40, 0, 128, 32, 32, 1, 1, "none"),
    "c64_cin24": (3, 24, 0, 64, 32, 32, 0, 1, "none"),
    "c64_cin64": (3, 64, 0, 64, 32, 32, 0, 1, "same"),
    "c64_up": (3, 64, 0, 64, 32, 32, 1, 1, "none"),
    "split": (3, 64, 0, 128, 16, 16, 0, 1, "none"),
    "split_cin40_down": (3, 40, 0, 128, 16, 16, 0, 1, "down"),
    "split_noact": (3, 64, 0, 128, 16, 16, 0, 0, "same"),
}


@pytest.fixture(scope="module")
def lib():
    import importlib
    L = importlib.import_module("m-cedm_amd.lib")
    L.load()
    return L


def dev(t):
    return None if t is None else t.cuda().contiguous()


def inputs(name):
    B, Ca, Cb, Cout, H, W, up, act, res = CASES[name]
    tag, Cin = "wino_addr/" + name, Ca + Cb
    hs, ws = (H // 2, W // 2) if up else (H, W)
    coef = torch.stack([fx.randn(tag + "/m", B, Cin) * 0.1, 1 + 0.1 * fx.randn(tag + "/s", B, Cin), 0.1 * fx.randn(tag + "/o", B, Cin),
                        torch.zeros(B, Cin)], -1) if act else None
    r = None if res == "none" else fx.randn(tag + "/res", B, Cout, *((H, W) if res == "same" else (2 * H, 2 * W)))
    return dict(xa=fx.randn(tag + "/xa", B, Ca, hs, ws), xb=fx.randn(tag + "/xb", B, Cb, hs, ws) if Cb else None,
                w=fx.randn(tag + "/w", Cout, Cin, 3, 3) / (Cin * 9) ** 0.5, b=fx.randn(tag + "/b", Cout) * 0.1, coef=coef, res=r)


def activated64(t, act, up):
    x = (torch.cat([t["xa"], t["xb"]], 1) if t["xb"] is not None else t["xa"]).double()
    if t["coef"] is not None:
        c = t["coef"].double()
        x = (x - c[..., 0, None, None]) * c[..., 1, None, None] + c[..., 2, None, None]
    if act:
        x = torch.nn.functional.silu(x)
    return torch.nn.functional.interpolate(x, scale_factor=2, mode="nearest") if up else x


def records(gsum, B, H, W, C):
    tiles = (H // 8) * (W // 16)
    return gsum[:B * tiles * (C // 4) * 2].view(B, tiles, C // 4, 2)


def profiled(L, fn):
    L.prof_enable(True)
    try:
        out = fn()
        torch.cuda.synchronize()
        names = sorted({r["name"] for r in L.prof_report()})
    finally:
        L.prof_enable(False)
    return out, names


def run(L, name, which):
    """which = 'new': the kernel under test; 'wino1': conv_wino1_kernel on the same values (output channels zero-padded to 128)."""
    B, Ca, Cb, Cout, H, W, up, act, res = CASES[name]
    t = inputs(name)
    Cp = 128 if which == "wino1" else Cout
    pad = lambda v, dim: None if v is None else torch.cat([v, torch.zeros(*v.shape[:dim], Cp - Cout, *v.shape[dim + 1:])], dim) if Cp != Cout else v
    args = (dev(t["xa"]), dev(t["xb"]), L.op_pack_conv_wino(dev(pad(t["w"], 0))), dev(pad(t["b"], 0)), Cp)
    kw = dict(coef=dev(t["coef"]), act=act, res=dev(pad(t["res"], 1)), res_mode=RS_DOWN if res == "down" else RS_NONE, want_sums=True)
    if which == "new" and name.startswith("split"):
        fn = lambda: L.op_conv_wino_split(*args, **kw)
    else:
        fn = lambda: L.op_conv_wino(*args, resample=RS_UP if up else RS_NONE, **kw)
    L.set_conv_wino1(1 if which == "wino1" else 0)
    try:
        (out, gsum), names = profiled(L, fn)
    finally:
        L.set_conv_wino1(-1)
    return out.cpu()[:, :Cout], records(gsum, B, H, W, Cp).cpu()[:, :, :Cout // 4], names


@pytest.mark.parametrize("name", list(CASES))
def test_outputs_and_records_equal_the_one_wave_kernel(lib, name):
    a, ra, na = run(lib, name, "new")
    b, rb, nb = run(lib, name, "wino1")
    Cout, up, act = CASES[name][3], CASES[name][6], CASES[name][7]
    cfg = "WinoSplitCfg" if name.startswith("split") else f"WinoCfg<{Cout // 32}>"
    want = f"conv_wino_kernel<{cfg}, {'true' if up else 'false'}, {'true' if act or up else 'false'}{', WinoUp<true>' if up else ''}>"
    assert na == [want], na
    assert len(nb) == 1 and nb[0].startswith("conv_wino1_kernel"), nb
    print(f"{name}: {int((a != b).sum())} of {a.numel()} outputs differ, max |d| {float((a - b).abs().max()):.3e}; "
          f"{int((ra != rb).sum())} of {ra.numel()} record values differ")
    assert torch.isfinite(a).all() and rb.abs().max() > 0
    assert torch.equal(a, b)
    assert torch.equal(torch.signbit(a), torch.signbit(b))
    assert torch.equal(ra, rb)


@pytest.mark.parametrize("name", ["up", "up_cin40", "c64_up"])
def test_up_sampling_form_vs_fp64(lib, name):
    B, Ca, Cb, Cout, H, W, up, act, res = CASES[name]
    t = inputs(name)
    out, _, _ = run(lib, name, "new")
    ref = torch.nn.functional.conv2d(activated64(t, act, up), t["w"].double(), t["b"].double(), padding=1)
    worst = _tol.close_per_entry(out, ref, what=f"{name}: up-sampled Winograd conv vs fp64", time_dim=0)
    print(f"{name}: worst err / bar {worst:.3f}")


# the SKIP form: (Cin, sk_Ca, sk_Cb) -- the 64 + 64 projection behind eight stages per tile (the two-stage trip), and five stages (the one-stage trip)
@pytest.mark.parametrize("Cin,sa,sb", [(128, 64, 64), (72, 32, 0)])
def test_skip_form_vs_fp64(lib, Cin, sa, sb):
    B, Cout, H, W = 3, 128, 32, 32
    tag = f"wino_addr/skip{Cin}_{sa}_{sb}"
    x = fx.randn(tag + "/x", B, Cin, H, W)
    w, b = fx.randn(tag + "/w", Cout, Cin, 3, 3) / (Cin * 9) ** 0.5, fx.randn(tag + "/b", Cout) * 0.1
    ws, bs = fx.randn(tag + "/ws", Cout, sa + sb, 1, 1) / (sa + sb) ** 0.5, fx.randn(tag + "/bs", Cout) * 0.1
    ska, skb = fx.randn(tag + "/ska", B, sa, H, W), (fx.randn(tag + "/skb", B, sb, H, W) if sb else None)
    coef = torch.stack([fx.randn(tag + "/m", B, Cin) * 0.1, 1 + 0.1 * fx.randn(tag + "/s", B, Cin), 0.1 * fx.randn(tag + "/o", B, Cin),
                        torch.zeros(B, Cin)], -1)
    wpk, bpk = lib.op_pack_conv(dev(w), dev(b))
    swpk, sbpk = lib.op_pack_conv(dev(ws), dev(bs))
    out, names = profiled(lib, lambda: lib.op_conv_skip(
        dev(x), wpk, lib.op_pack_conv_wino(dev(w)), bpk, Cout, coef=dev(coef), sk_xa=dev(ska), sk_xb=dev(skb), sk_wpk=swpk,
        sk_wfrag=lib.op_pack_conv_frag(dev(ws)), sk_bias=sbpk))
    assert names == ["conv_wino_kernel<WinoSkipCfg<4>, false, true>"], names
    sk = (torch.cat([ska, skb], 1) if sb else ska).double()
    ref = torch.nn.functional.conv2d(activated64(dict(xa=x, xb=None, coef=coef), 1, 0), w.double(), b.double(), padding=1) + \
        torch.nn.functional.conv2d(sk, ws.double(), bs.double())
    worst = _tol.close_per_entry(out.cpu(), ref, what=f"SKIP form {Cin} + ({sa} + {sb}) vs fp64", time_dim=0)
    print(f"skip {Cin} + ({sa} + {sb}): worst err / bar {worst:.3f}")
