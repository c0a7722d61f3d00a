"""Cases, inputs, the fp64 reference and the device runs of tests/test_hip_wino_upz.py, shared with its child process: run as a
program (python tests/_wino_upz.py OUT.npz) this file IS the child -- the same calls on the same fx.randn inputs under whatever
MCEDM_WINO_PER the environment carries (the library reads it once per process), stored in an .npz.

A case is conv0 of an up block: out = conv3x3(up2x(act(coef(cat(xa, xb))))) + bias (+ up2x(res)), with the fused GroupNorm records.
  on : the zero-position variant (conv_wino_kernel<WinoCfg<MB>, true, true, WinoUp<true>>: 9 of the 16 Winograd positions, the input staged
       and transformed at source resolution);
  pos: its positions on the sixteen-position kernel's staging (WinoUp<false>; switch value 2, kept for A/B runs);
  off: all sixteen positions (conv_wino_kernel<WinoCfg<MB>, true, true>)."""
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import fixtures as fx  # noqa: E402
from oracle import mcedm_oracle as orc  # noqa: E402

RS_NONE, RS_UP = 0, 1
TILE_H, TILE_W = 8, 16                    # WPH x WPW of csrc/conv_wino.hpp: one pixel tile
FORCED = 2                                # tiles per workgroup of the child, where it divides the tiles per image

# name: (B, Ca, Cb, Cout, H, W, act, coef, res); (H, W) is the output size, the sources are (H / 2, W / 2)
CASES = {
    "tiles_2x2": (2, 128, 0, 128, 16, 32, 1, True, False),     # 2 x 2 tiles: all four borders and both inner tile edges
    "two_sources": (1, 64, 64, 128, 16, 16, 1, True, False),
    "odd_chunks": (2, 24, 0, 128, 24, 16, 1, True, False),     # three chunks: a half-empty last stage; three tiles per image
    "two_blocks": (2, 128, 0, 256, 16, 16, 1, True, False),    # two output-channel blocks
    "c64": (2, 64, 0, 64, 16, 32, 1, True, False),             # the 256-thread WinoCfg<2> (one chunk per stage)
    "noact": (2, 64, 0, 128, 16, 32, 0, False, False),         # act = 0 and no coefficient table
    "up_res": (2, 128, 0, 128, 16, 32, 1, True, True),         # plus the RS_UP residual
}


def kernels(name):
    """{arm: the profiler's name of its kernel}."""
    mb = 4 if CASES[name][3] % 128 == 0 else 2
    return {"on": f"conv_wino_kernel<WinoCfg<{mb}>, true, true, WinoUp<true>>", "pos": f"conv_wino_kernel<WinoCfg<{mb}>, true, true, WinoUp<false>>",
            "off": f"conv_wino_kernel<WinoCfg<{mb}>, true, true>"}


def tiles(name):
    """(tiles in the launch, tiles per image)."""
    B, H, W = CASES[name][0], CASES[name][4], CASES[name][5]
    per_img = (H // TILE_H) * (W // TILE_W)
    return B * per_img, per_img


def case_inputs(name):
    B, Ca, Cb, Cout, H, W, act, use_coef, res = CASES[name]
    tag, Cin, hs, ws = "wino_upz/" + name, Ca + Cb, H // 2, W // 2
    coef = torch.stack([fx.randn(tag + "/m", B, Cin) * 0.1, 1 + 0.1 * fx.randn(tag + "/s", B, Cin), 0.1 * fx.randn(tag + "/o", B, Cin),
                        torch.zeros(B, Cin)], -1) if use_coef else None
    return dict(xa=fx.randn(tag + "/xa", B, Ca, hs, ws), xb=fx.randn(tag + "/xb", B, Cb, hs, ws) if Cb else None,
                w=fx.randn(tag + "/w", Cout, Cin, 3, 3) / (Cin * 9) ** 0.5, b=fx.randn(tag + "/b", Cout) * 0.1, coef=coef,
                res=fx.randn(tag + "/res", B, Cout, hs, ws) if res else None)


def case_reference(name, t):
    """fp64: nearest up-sampling of the activated source, torch's direct convolution, the up-sampled residual."""
    B, Ca, Cb, Cout, H, W, act, use_coef, res = CASES[name]
    x = (torch.cat([t["xa"], t["xb"]], 1) if Cb else t["xa"]).double()
    if use_coef:
        c = t["coef"].double()
        x = (x - c[..., 0, None, None]) * c[..., 1, None, None] + c[..., 2, None, None]
    if act:
        x = torch.nn.functional.silu(x)
    ref = torch.nn.functional.conv2d(orc.resample_up(x), t["w"].double(), t["b"].double(), padding=1)
    return ref + orc.resample_up(t["res"].double()) if res else ref


def dev(t):
    return None if t is None else t.cuda().contiguous()


def profiled(L, total_tiles, fn):
    """fn() with the launch profiler and the conv debug records on -> (result, kernel names, word 4 = tiles per workgroup of the
    records that the one-tile-per-workgroup grid would write)."""
    buf = torch.zeros(total_tiles, 16, dtype=torch.int64, device="cuda")
    L.set_conv_debug(buf)
    L.prof_enable(True)
    try:
        out = fn()
        torch.cuda.synchronize()
        names = sorted({r["name"] for r in L.prof_report()})
    finally:
        L.prof_enable(False)
        L.set_conv_debug(None)
    return out, names, buf[:, 4].cpu().numpy()


def run_case(L, name):
    t = case_inputs(name)
    B, Ca, Cb, Cout, H, W, act, use_coef, res = CASES[name]
    wino = L.op_pack_conv_wino(dev(t["w"]))
    args = (dev(t["xa"]), dev(t["xb"]), wino, dev(t["b"]), Cout)
    kw = dict(coef=dev(t["coef"]), act=act, resample=RS_UP, res=dev(t["res"]), res_mode=RS_UP if res else RS_NONE, want_sums=True)
    r = {}
    for key, flag in (("on", 1), ("pos", 2), ("off", 0)):
        L.set_conv_wino_upz(flag)
        try:
            (out, sums), names, per = profiled(L, tiles(name)[0], lambda: L.op_conv_wino(*args, **kw))
        finally:
            L.set_conv_wino_upz(-1)
        r[f"{name}/{key}/out"], r[f"{name}/{key}/sums"] = out.cpu().numpy(), sums.cpu().numpy()
        r[f"{name}/{key}/names"], r[f"{name}/{key}/per"] = np.array(names), per
    return r


def run_all(L):
    r = {}
    for name in CASES:
        r.update(run_case(L, name))
    return r


if __name__ == "__main__":
    lib = importlib.import_module("m-cedm_amd.lib")
    lib.load()
    np.savez(sys.argv[1], **run_all(lib))
