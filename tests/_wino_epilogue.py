"""Cases, inputs and device runs of tests/test_hip_wino_epilogue.py, shared with its child process: run as a program
(python tests/_wino_epilogue.py OUT.npz) this file IS the child -- the four residual modes at B = 2, 64 x 64 under whatever
MCEDM_WINO_PER the environment carries (the library reads it once per process), on conv_wino_kernel and on conv_wino1_kernel:
outputs, records and the tiles per workgroup that every workgroup recorded, stored in an .npz."""
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import fixtures as fx  # noqa: E402
from tests import _wino_per as WP  # noqa: E402

RS_NONE, RS_UP, RS_DOWN = 0, 1, 2
RES_MODES = ("none", "same", "up", "down")
RES_MODE = {"none": RS_NONE, "same": RS_NONE, "up": RS_UP, "down": RS_DOWN}
PER_SHAPE = (2, 32, 128, 64, 64)          # B, Cin, Cout, H, W of the forced-schedule runs: 32 tiles per image


def res_shape(res, H, W):
    return {"none": None, "same": (H, W), "up": (H // 2, W // 2), "down": (2 * H, 2 * W)}[res]


def make_inputs(tag, B, Ca, Cb, Cout, H, W, act, res):
    """fx.randn inputs of one launch: a transform row per (sample, channel) where the launch has an activation"""
    Cin, rs = Ca + Cb, res_shape(res, H, W)
    return dict(xa=fx.randn(tag + "/xa", B, Ca, H, W), xb=fx.randn(tag + "/xb", B, Cb, H, W) if Cb else None,
                w=fx.randn(tag + "/w", Cout, Cin, 3, 3) / (Cin * 9) ** 0.5, b=fx.randn(tag + "/b", Cout) * 0.1,
                coef=WP.coef_table(tag, B, Cin) if act else None, res=fx.randn(tag + "/res", B, Cout, *rs) if rs else None)


def launch(L, t, Cout, act, res, rc, wino1=False, split=False, pad_to=None):
    """One launch -> (out [B, Cout, H, W], records [B, tiles, Cout / rc, 2], kernel names).  rc = 4: op_conv_wino(.., want_sums=True);
    rc = 2: op_conv_sums, the dispatcher with records of two channels (it takes the Winograd kernel for these shapes; the names
    prove it).  pad_to: output channels zero-padded to that many (a channel's sums never depend on the launch's other channels)."""
    Cp = pad_to or Cout
    pad = lambda v, dim: None if v is None else torch.cat([v, torch.zeros(*v.shape[:dim], Cp - Cout, *v.shape[dim + 1:])], dim) if Cp != Cout else v
    w, b, r = WP.dev(pad(t["w"], 0)), WP.dev(pad(t["b"], 0)), WP.dev(pad(t["res"], 1))
    xa, xb, coef = WP.dev(t["xa"]), WP.dev(t["xb"]), WP.dev(t["coef"])
    wino = L.op_pack_conv_wino(w)
    kw = dict(coef=coef, act=act, res=r, res_mode=RES_MODE[res])
    if split:
        assert rc == 4
        fn = lambda: L.op_conv_wino_split(xa, xb, wino, b, Cp, want_sums=True, **kw)
    elif rc == 4:
        fn = lambda: L.op_conv_wino(xa, xb, wino, b, Cp, want_sums=True, **kw)
    else:
        wpk, bpk = L.op_pack_conv(w, b)
        fn = lambda: L.op_conv_sums(xa, xb, wpk, bpk, Cp, 3, rc=rc, wino=wino, **kw)[:2]
    L.set_conv_wino1(1 if wino1 else 0)
    L.prof_enable(True)
    try:
        out, gsum = fn()
        torch.cuda.synchronize()
        names = sorted({r_["name"] for r_ in L.prof_report()})
    finally:
        L.prof_enable(False)
        L.set_conv_wino1(-1)
    B, _, H, W = out.shape
    tiles = (H // WP.TILE_H) * (W // WP.TILE_W)
    rec = gsum[:B * tiles * (Cp // rc) * 2].view(B, tiles, Cp // rc, 2)
    return out.cpu()[:, :Cout], rec.cpu()[:, :, :Cout // rc], names


def run_per(L):
    """The four residual modes at PER_SHAPE on both kernels, records of four channels."""
    B, Cin, Cout, H, W = PER_SHAPE
    r = {}
    for res in RES_MODES:
        t = make_inputs("wino_epilogue/per_" + res, B, Cin, 0, Cout, H, W, 1, res)
        for wino1 in (False, True):
            key = res + ("@wino1" if wino1 else "")
            (out, rec, names), per = WP.recorded(L, WP.n_tiles(B, H, W), lambda: launch(L, t, Cout, 1, res, 4, wino1=wino1))
            r[key + "/out"], r[key + "/rec"], r[key + "/per"] = out.numpy(), rec.numpy(), per
            r[key + "/names"] = np.array(names)
    return r


if __name__ == "__main__":
    lib = importlib.import_module("m-cedm_amd.lib")
    lib.load()
    np.savez(sys.argv[1], **run_per(lib))
