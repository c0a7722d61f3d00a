"""Cases, inputs, references and the device runs of tests/test_hip_wino_per.py, shared with its child processes: run as a
program (python tests/_wino_per.py OUT.npz) this file IS the child -- the same calls on the same fx.randn inputs under whatever
MCEDM_WINO_PER the environment carries (the library reads it once per process), outputs and the tiles per workgroup that every
workgroup recorded (word 4 of its debug record, csrc/conv_wino.hip, csrc/conv_wino1.hip) stored in an .npz."""
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

RS_NONE, RS_UP, RS_DOWN = 0, 1, 2
TILE_H, TILE_W = 8, 16                    # WPH x WPW of csrc/conv_wino.hpp: one pixel tile

# name: (B, Ca, Cb, Cout, H, W, act, coef, up, res); (H, W) is the conv (= output) size; res: None, "same", "up" (the residual is
# up-sampled from half size) or "down" (2 x 2 mean of a double-size source).  4 or 8 tiles per image each: 2 and 4 both divide.
CASES = {
    "c128_res": (2, 128, 0, 128, 16, 32, 1, True, False, "same"),    # 4 / 2 workgroups: not a multiple of 8 (the lid fallback)
    "odd_chunks": (4, 24, 0, 128, 32, 16, 0, True, False, None),     # 3 chunks: a half-empty last stage; one tile column; 8 workgroups at per = 2
    "one_stage_128": (2, 8, 0, 128, 16, 32, 1, False, False, None),  # one stage per tile: a tile boundary at every barrier
    "one_stage_64": (2, 8, 0, 64, 16, 32, 1, False, False, None),    # ... of WinoCfg<2> (one chunk per stage)
    "concat_64": (2, 64, 64, 64, 16, 64, 1, True, False, None),      # WinoCfg<2>, 8 tiles per image, two input tensors
    "noact_192": (3, 16, 0, 192, 16, 32, 0, False, False, None),     # conv_wino_kernel<C, false, false>, three output-channel blocks
    "c256_res": (4, 128, 128, 256, 16, 32, 1, True, False, "same"),  # 32 chunks, two output-channel blocks
    "up": (2, 128, 0, 128, 32, 32, 1, True, True, None),             # up-sampled from 16 x 16, 8 tiles per image
    "up_res": (2, 128, 0, 128, 32, 32, 1, True, True, "up"),         # ... plus an RS_UP residual
    "down_res": (2, 128, 0, 128, 16, 32, 1, True, False, "down"),    # RS_DOWN residual from a (2, 128, 32, 64) source
}
WINO1_CASES = ("c128_res", "up", "up_res", "down_res")             # rerun on conv_wino1_kernel: bit-equal to WinoCfg<4>
# the Winograd kernel as a data gradient: (B, Cin, Cout, H, W) of the FORWARD conv
DGRAD_CASES = {
    "dgrad_128": (2, 128, 128, 16, 32),
    "dgrad_64": (2, 64, 128, 16, 32),          # 64 gradient channels: WinoCfg<2>
    "dgrad_odd": (3, 128, 24, 24, 16),         # odd chunk count
    "dgrad_one": (1, 64, 8, 8, 16),            # one chunk, one tile
}
DGRAD_FORCED = ("dgrad_128", "dgrad_64")     # four tiles per image: also run under a forced schedule
SEAM = (2, 24, 128, 32, 16)                  # B, Cin, Cout, H, W of the exact test


def n_tiles(B, H, W):
    return B * (H // TILE_H) * (W // TILE_W)


def coef_table(tag, B, C):
    return torch.stack([fx.randn(tag + "/m", B, C) * 0.1, 1 + 0.1 * fx.randn(tag + "/s", B, C), 0.1 * fx.randn(tag + "/o", B, C),
                        torch.zeros(B, C)], -1)


def case_inputs(name):
    B, Ca, Cb, Cout, H, W, act, use_coef, up, res = CASES[name]
    tag, Cin = "wino_per/" + name, Ca + Cb
    hs, ws = (H // 2, W // 2) if up else (H, W)
    rshape = {None: None, "same": (H, W), "up": (H // 2, W // 2), "down": (2 * H, 2 * W)}[res]
    return dict(xa=fx.randn(tag + "/xa", B, Ca, hs, ws), xb=fx.randn(tag + "/xb", B, Cb, hs, ws) if Cb else None,
                w=fx.randn(tag + "/w", Cout, Cin, 3, 3) / (Cin * 9) ** 0.5, b=fx.randn(tag + "/b", Cout) * 0.1,
                coef=coef_table(tag, B, Cin) if use_coef else None,
                res=fx.randn(tag + "/res", B, Cout, *rshape) if rshape else None)


def case_reference(name, t):
    """fp64: torch's direct convolution of the transformed, resampled input, plus the resampled residual."""
    B, Ca, Cb, Cout, H, W, act, use_coef, up, res = CASES[name]
    x = (torch.cat([t["xa"], t["xb"]], 1) if Cb else t["xa"]).double()
    if use_coef:
        c = t["coef"].double()
        x = (x - c[..., 0, None, None]) * c[..., 1, None, None] + c[..., 2, None, None]
    if act:
        x = torch.nn.functional.silu(x)
    if up:
        x = orc.resample_up(x)
    ref = torch.nn.functional.conv2d(x, t["w"].double(), t["b"].double(), padding=1)
    if res == "same":
        ref = ref + t["res"].double()
    elif res == "up":
        ref = ref + orc.resample_up(t["res"].double())
    elif res == "down":
        ref = ref + orc.resample_down(t["res"].double())
    return ref


def dgrad_inputs(name):
    B, Cin, Cout, H, W = DGRAD_CASES[name]
    tag = "wino_per/" + name
    return dict(w=fx.randn(tag + "/w", Cout, Cin, 3, 3) / (Cin * 9) ** 0.5, dy=fx.randn(tag + "/dy", B, Cout, H, W))


def dgrad_reference(name, t):
    B, Cin, Cout, H, W = DGRAD_CASES[name]
    u = fx.randn("wino_per/" + name + "/u", B, Cin, H, W).double().requires_grad_(True)
    (gu,) = torch.autograd.grad(torch.nn.functional.conv2d(u, t["w"].double(), padding=1), u, t["dy"].double())
    return gu


def seam_inputs():
    """Integers: x in {-3 .. 3}, w in {-2 .. 2} (see test_exact_inputs_stay_exact_in_fp32_winograd_arithmetic)."""
    B, Cin, Cout, H, W = SEAM
    x = np.round(fx.uniform("wino_per/seam/x", B, Cin, H, W) * 3.0)
    w = np.round(fx.uniform("wino_per/seam/w", Cout, Cin, 3, 3) * 2.0)
    return dict(x=torch.from_numpy((x + 0.0).astype(np.float32)), w=torch.from_numpy((w + 0.0).astype(np.float32)))


def seam_reference(t):
    return torch.nn.functional.conv2d(t["x"].double(), t["w"].double(), padding=1)


def dev(t):
    return None if t is None else t.cuda().contiguous()


def recorded(L, total_tiles, fn):
    """fn() with the conv debug records switched on for it alone -> (its result, word 4 of each of the total_tiles records that
    the one-tile-per-workgroup grid would write; a workgroup that did not run leaves its zero)."""
    buf = torch.zeros(total_tiles, 16, dtype=torch.int64, device="cuda")
    L.set_conv_debug(buf)
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        L.set_conv_debug(None)
    return out, buf[:, 4].cpu().numpy()


def run_case(L, name, t, wino1=False):
    B, Ca, Cb, Cout, H, W, act, use_coef, up, res = CASES[name]
    wino = L.op_pack_conv_wino(dev(t["w"]))
    args = (dev(t["xa"]), dev(t["xb"]), wino, dev(t["b"]), Cout)
    kw = dict(coef=dev(t["coef"]), act=act, resample=RS_UP if up else RS_NONE, res=dev(t["res"]),
              res_mode={None: RS_NONE, "same": RS_NONE, "up": RS_UP, "down": RS_DOWN}[res])
    if wino1:
        L.set_conv_wino1(1)
    try:
        out, per = recorded(L, n_tiles(B, H, W), lambda: L.op_conv_wino(*args, **kw))
    finally:
        if wino1:
            L.set_conv_wino1(-1)
    return out.cpu().numpy(), per


def run_dgrad(L, name, t):
    B, Cin, Cout, H, W = DGRAD_CASES[name]
    table = L.op_pack_conv_wino(dev(t["w"]), dgrad=True)
    out, per = recorded(L, n_tiles(B, H, W), lambda: L.op_conv_wino(dev(t["dy"]), None, table, None, Cin))
    return out.cpu().numpy(), per


def run_seam(L, t):
    B, Cin, Cout, H, W = SEAM
    wino = L.op_pack_conv_wino(dev(t["w"]))
    out, per = recorded(L, n_tiles(B, H, W), lambda: L.op_conv_wino(dev(t["x"]), None, wino, None, Cout))
    return out.cpu().numpy(), per


def run_all(L):
    """Every device run of the forced-schedule tests -> {key + "/out": output, key + "/per": recorded tiles per workgroup}."""
    r = {}
    for name in CASES:
        t = case_inputs(name)
        r[name + "/out"], r[name + "/per"] = run_case(L, name, t)
        if name in WINO1_CASES:
            r[name + "@wino1/out"], r[name + "@wino1/per"] = run_case(L, name, t, wino1=True)
    for name in DGRAD_FORCED:
        r[name + "/out"], r[name + "/per"] = run_dgrad(L, name, dgrad_inputs(name))
    r["seam/out"], r["seam/per"] = run_seam(L, seam_inputs())
    return r


def total_tiles_of(key):
    name = key.split("@")[0]
    if name == "seam":
        B, _, _, H, W = SEAM
    elif name in DGRAD_CASES:
        B, _, _, H, W = DGRAD_CASES[name]
    else:
        B, H, W = CASES[name][0], CASES[name][4], CASES[name][5]
    return n_tiles(B, H, W)


if __name__ == "__main__":
    lib = importlib.import_module("m-cedm_amd.lib")
    lib.load()
    np.savez(sys.argv[1], **run_all(lib))
