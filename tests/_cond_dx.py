"""What tools/make_golden_cond_ddim_dx.py (the reference's PlCondDdim with ``dx_cond: True``, CPU) and the tests of dx_cond on
PlCondDdim (tests/test_cond_dx_cpu.py, tests/test_hip_cond_dx.py) share: the network configurations, the cases, the tagged inputs
and the draws.  Sampler cases, inputs, draws and the comparison bar are tests/_cond_guided.py's.  Only the reference's outputs live in
tests/golden/cond_ddim_dx_{cat,enc,guided}.npz."""
import dataclasses
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import fixtures as fx  # noqa: E402
from oracle import mcedm_oracle as orc  # noqa: E402
from tests import _cond_guided as G  # noqa: E402

SEED = 17                                      # tools/make_golden_cond_ddim.SEED
MODES = ("cat", "enc")
# the self-conditioning network's table (tools/make_golden_cond_ddim.CFG) with the dx input on top
BASE_CFG = orc.UNetConfig(in_channels=1, cond_channels=2, out_ch=1)
B, H, W = G.B, G.H, G.W
# One file per group, each under 1 MB: a mode's sampler trajectories, the network forward and -- where there is room -- the
# training step; the guided cases (enc only) carry the training step of the enc network.
GOLDEN = {"cat": "cond_ddim_dx_cat.npz", "enc": "cond_ddim_dx_enc.npz", "guided": "cond_ddim_dx_guided.npz"}
TRAIN_FILE = {"cat": "cat", "enc": "guided"}
SAMPLER_TAGS = ("ddim", "ddim_cfg_eta", "vp", "vp_churn_cfg")
GUIDED_TAGS = ("ddim_cfg_eta", "vp", "darcy")  # enc mode, guide_dx on top (darcy: the route only, see the generator)
# (dx draw, cond_p draw, self-conditioning draw) with cond_p = 0.8: dx on / off (> 0.1), cond on / off (< 0.8), pre-pass on / off (< 0.5)
BRANCHES = {"dx_cond_sc": (0.5, 0.1, 0.2), "dx_cond_nosc": (0.5, 0.1, 0.7), "nodx_cond_sc": (0.05, 0.1, 0.2),
            "dx_nocond_nosc": (0.5, 0.9, 0.7)}
GRAD_NAMES = ["enc.128x128_conv.weight", "enc.128x128_conv.bias", "out_conv.weight", "dec.32x32_in0.qkv.weight",
              "map_layer0.weight", "map_layer1.bias", "enc.32x32_down.norm0.weight"]      # tools/make_golden_cond_ddim.GRAD_NAMES
ENC_GRAD_NAMES = ["dx_enc.0.weight", "dx_enc.2.bias", "combine_enc.weight"]
# combine_enc.weight [64, 128, 3, 3] is 295 KB per branch: every 8th input channel of it is stored (both halves of cat(conv_in(.),
# dx_enc(dx)) are in it); the whole tensor is held by its squared norm
STORED_SLICE = {"combine_enc.weight": (slice(None), slice(None, None, 8))}
LABELS = (0.0, 1.0, 500.0, 999.0)


def cfg_of(mode):
    return dataclasses.replace(BASE_CFG, dx_channels=1, dx_mode=mode)


def grad_names(mode):
    return GRAD_NAMES + (ENC_GRAD_NAMES if mode == "enc" else [])


def stored(name, grad):
    """The part of a gradient that the fixture holds."""
    return grad[STORED_SLICE[name]] if name in STORED_SLICE else grad


def model_update(mode):
    """hparams.model entries on top of the self-conditioning configuration."""
    return dict(dx_cond=True, cat_dx=mode == "cat", dx_norm="prob", dx_detach=True, cond_p=0.8)


def net_inputs():
    """x, cond, x_self_cond, dx [4, 1, H, W] and the labels of the network-forward case."""
    x, cond, xsc, dx = (fx.randn(f"cdx/fwd/{k}", 4, 1, H, W) for k in ("x", "cond", "xsc", "dx"))
    return x, cond, xsc, dx * 0.1, torch.tensor(LABELS)


def sampler_key(mode, tag, guided=False):
    return f"{mode}{'_guided' if guided else ''}::{tag}"
