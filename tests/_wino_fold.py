"""Cases, inputs, the fp64 reference and the device runs of tests/test_hip_wino_fold.py, shared with its child process: run as a
program (python tests/_wino_fold.py OUT.npz) this file IS the child -- the same calls on the same fx.randn inputs under whatever
MCEDM_WINO_PER the environment carries (the library reads it once per process), stored in an .npz.

A case is conv1 of an un-resampled decoder block: out = conv3x3(silu(coef(h))) + bias + skip(cat(xa, xb)), skip a 1x1 conv.
  on : ONE launch_conv with the projection folded in (ConvArgs::sk_*, the Winograd kernel's SKIP variant computes it);
  off: the projection as a launch of its own (conv1x1_reg_kernel) whose result conv1 reads back as its residual."""
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import fixtures as fx  # noqa: E402

TILE_H, TILE_W = 8, 16                    # WPH x WPW of csrc/conv_wino.hpp: one pixel tile
FORCED = 4                                # tiles per workgroup of the child: divides the 8 / 16 tiles per image of every case

# name: (B, sk_Ca, sk_Cb, Cout, H, W); conv1 itself is Cout -> Cout.  32 x 32 is the smallest image on which both the Winograd
# kernel and conv1x1_reg_kernel serve the block.
CASES = {
    "b2_128_128": (2, 128, 128, 128, 32, 32),
    "b1_wide": (1, 128, 128, 128, 32, 64),     # 16 tiles per image, four tile columns
    "b3_64_192": (3, 64, 192, 128, 32, 32),    # the source changes after four of the sixteen stages; odd batch
    "b2_256_0": (2, 256, 0, 128, 32, 32),      # one source
}


def n_tiles(name):
    B, _, _, _, H, W = CASES[name]
    return B * (H // TILE_H) * (W // TILE_W)


def case_inputs(name):
    B, Ca, Cb, Cout, H, W = CASES[name]
    tag = "wino_fold/" + name
    coef = torch.stack([fx.randn(tag + "/m", B, Cout) * 0.1, 1 + 0.1 * fx.randn(tag + "/s", B, Cout), 0.1 * fx.randn(tag + "/o", B, Cout),
                        torch.zeros(B, Cout)], -1)
    return dict(h=fx.randn(tag + "/h", B, Cout, H, W), coef=coef,
                w=fx.randn(tag + "/w", Cout, Cout, 3, 3) / (Cout * 9) ** 0.5, b=fx.randn(tag + "/b", Cout) * 0.1,
                xa=fx.randn(tag + "/xa", B, Ca, H, W), xb=fx.randn(tag + "/xb", B, Cb, H, W) if Cb else None,
                ws=fx.randn(tag + "/ws", Cout, Ca + Cb, 1, 1) / (Ca + Cb) ** 0.5, bs=fx.randn(tag + "/bs", Cout) * 0.1)


def case_reference(t):
    """fp64: torch's direct convolution of the transformed input plus the 1x1 projection of the concatenated block input."""
    c = t["coef"].double()
    x = torch.nn.functional.silu((t["h"].double() - c[..., 0, None, None]) * c[..., 1, None, None] + c[..., 2, None, None])
    sk = torch.cat([t["xa"], t["xb"]], 1) if t["xb"] is not None else t["xa"]
    return (torch.nn.functional.conv2d(x, t["w"].double(), t["b"].double(), padding=1) +
            torch.nn.functional.conv2d(sk.double(), t["ws"].double(), t["bs"].double()))


def dev(t):
    return None if t is None else t.cuda().contiguous()


def profiled(L, total_tiles, fn):
    """fn() with the launch profiler and the conv debug records on -> (result, kernel names, word 4 = tiles per workgroup of the
    records that the one-tile-per-workgroup grid of the LAST conv launch would write)."""
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
    B, Ca, Cb, Cout, H, W = CASES[name]
    h, coef, xa, xb = dev(t["h"]), dev(t["coef"]), dev(t["xa"]), dev(t["xb"])
    wpk, bpk = L.op_pack_conv(dev(t["w"]), dev(t["b"]))
    wino = L.op_pack_conv_wino(dev(t["w"]))
    spk, sbias = L.op_pack_conv(dev(t["ws"]), dev(t["bs"]))
    sfrag = L.op_pack_conv_frag(dev(t["ws"]))
    r = {}

    def on():
        return L.op_conv_skip(h, wpk, wino, bpk, Cout, coef=coef, sk_xa=xa, sk_xb=xb, sk_wpk=spk, sk_wfrag=sfrag, sk_bias=sbias,
                              want_sums=True)

    def off():
        sk = L.op_conv(xa, xb, spk, sbias, Cout, 1)
        return L.op_conv_skip(h, wpk, wino, bpk, Cout, coef=coef, res=sk, want_sums=True)

    for key, fn in (("on", on), ("off", off)):
        (out, sums), names, per = profiled(L, n_tiles(name), fn)
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
