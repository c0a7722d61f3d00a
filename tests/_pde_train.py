"""Shared by tools/make_golden_pde_train.py, tests/test_pde_train_cpu.py and tests/test_hip_pde_train.py: the case table of the PDE
training term (PlCondEdm.training_step with pde_loss_lambda > 0, models/ddim.py:1726-1731), its inputs, and a torch-autograd
restatement of the term built from oracle/pde_oracle.py.  The restatement is pinned in fp32 against the reference's own
get_pde_loss (tests/golden/pde_train.npz); run in float64 it is the second reference of the GPU tests."""
import numpy as np
import torch

from oracle import fixtures as fx
from oracle import pde_oracle as po

NORM_STATS = (1.4, 0.05, 0.0, 0.1)            # input mean / std, target mean / std: the un-normalised h (or a) stays positive
SYSTEMS = {"swe": dict(Tn=1.28, x_min=-2.5, x_max=2.5), "swe_per": dict(Tn=0.128, x_min=-0.5, x_max=0.5), "darcy": {}}
# (B, T, X): one row (no stepped row: value 0 and gradient 0 when gt is the state itself; with use_gt_pde only row 0's own term); replicate boundary with all three neighbours on one cell; cells that
# cross a 256-thread block and leave a ragged tail
SWE_SHAPES = [(3, 8, 16), (2, 1, 5), (1, 2, 1), (2, 3, 3), (2, 3, 70), (5, 7, 37)]
DEGENERATE = {(2, 1, 5)}
DARCY_SIZES = [5, 8, 19]
# amplitude of D per system / size: chosen so that the REFERENCE clamps between 10 % and 90 % of the cells (the tool asserts it)
AMP = {"swe": 0.6, "swe_per": 0.6, 5: 1.0, 8: 1.0, 19: 0.6}
# input tags that were redrawn until no cell of the reference's residual lies within 1e-3 of the clamp (fp32 rounding could move it)
RETRY = {"swe/5x7x37/gt": 1, "swe_per/2x3x70/gt": 2, "swe_per/5x7x37": 1, "swe_per/5x7x37/gt": 2, "swe_per/1x2x1/gt": 2}


def _cases():
    c = {}
    for system in ("swe", "swe_per"):
        for (B, T, X) in SWE_SHAPES:
            for use_gt in (False, True):
                for prop_t in (False, True):
                    name = f"{system}_{B}x{T}x{X}_{'gt' if use_gt else 'self'}{'_propt' if prop_t else ''}"
                    c[name] = dict(system=system, B=B, H=T, W=X, use_gt=use_gt, prop_t=prop_t, dry=False,
                                   degenerate=(B, T, X) in DEGENERATE and not use_gt, one_row=(B, T, X) in DEGENERATE, tag=f"{system}/{B}x{T}x{X}", amp=AMP[system])
    for S in DARCY_SIZES:
        for prop_t in (False, True):
            c[f"darcy_S{S}{'_propt' if prop_t else ''}"] = dict(system="darcy", B=3, H=S, W=S, use_gt=False, prop_t=prop_t, dry=False,
                                                                degenerate=False, one_row=False, tag=f"darcy/{S}", amp=AMP[S])
    # a dry cell: h + 1e-8 == 0 in fp32.  h = -1e-8 is not on the fp32 grid around the mean of NORM_STATS, so this case un-normalises
    # h with (0, 1) and carries the physical depth in the "normalised" field.  Whatever the reference returns there is expected.
    c["swe_per_dry"] = dict(system="swe_per", B=2, H=4, W=9, use_gt=False, prop_t=False, dry=True, degenerate=False,
                            one_row=False, tag="swe_per/dry", amp=AMP["swe_per"])
    for v in c.values():
        v["stats"] = (0.0, 1.0, 0.0, 0.1) if v["dry"] else NORM_STATS
    return c


OP_CASES = _cases()


def op_inputs(name):
    """(h, D, gt, sigma): h normalised (B, H, W, 1), D (B, 1, H, W), gt un-normalised (B, H, W, 2) or None, sigma (B, 1, 1, 1) or None."""
    c = OP_CASES[name]
    B, H, W = c["B"], c["H"], c["W"]
    tag = c["tag"] + ("/gt" if c["use_gt"] else "")
    tag += f"/retry{RETRY[tag]}" if tag in RETRY else ""
    st = c["stats"]
    h = fx.randn(f"pde_train/{tag}/h", B, H, W, 1)
    D = fx.randn(f"pde_train/{tag}/D", B, 1, H, W) * c["amp"]
    if c["dry"]:
        h = h * 0.05 + 1.4
        h[1, 1, 4, 0] = -1e-8
        assert float(h[1, 1, 4, 0] + 1e-8) == 0.0
    gt = None
    if c["use_gt"]:
        gt = torch.cat([h * st[1] + st[0], D.permute(0, 2, 3, 1) * st[3] + st[2]], dim=-1)
        gt = (gt + fx.randn(f"pde_train/{tag}/gt", B, H, W, 2) * torch.tensor([0.3 * st[1], 0.3 * st[3]])).contiguous()
    sigma = (fx.randn(f"pde_train/{tag}/sigma", B, 1, 1, 1) * 1.2 - 1.2).exp() if c["prop_t"] else None
    return h, D, gt, sigma


def residual_matrix(system, x_unnorm, gt_unnorm, stats=NORM_STATS):
    """The clamped (b, t, x) residual of get_pde_loss (models/ddim.py:1405-1411) from oracle/pde_oracle.py."""
    if system == "darcy":
        return po.darcy_residual(x_unnorm, clamp_loss=True)
    kw = SYSTEMS[system]
    dt = x_unnorm.dtype
    return po.swe_fv_residual(x_unnorm, gt_unnorm, torch.tensor(stats[1], dtype=torch.float32).to(dt),
                              torch.tensor(stats[3], dtype=torch.float32).to(dt), kw["Tn"], kw["x_min"], kw["x_max"],
                              clamp_loss=True).sum(dim=-1)


def restate(system, h, D, gt=None, sigma=None, dtype=torch.float32, stats=NORM_STATS):
    """(pde_loss, d pde_loss / d D) of get_pde_loss(h, D, gt, sigma, clamp_loss=True), models/ddim.py:1388-1422, by autograd.
    gt None: the target IS x_unnorm (the same tensor, :1402-1403), so the gradient flows through it too.  sigma divides the
    (b, t, x) matrix as (b, 1, 1, 1) (:1415-1416), which broadcasts to (b, b, t, x): every sample meets every noise level."""
    f32 = lambda v: torch.tensor(v, dtype=torch.float32).to(dtype)            # the normalisers hold fp32 statistics
    with torch.enable_grad():
        Dl = D.detach().to(dtype).requires_grad_(True)
        x = torch.cat([h.to(dtype) * f32(stats[1]) + f32(stats[0]), Dl.permute(0, 2, 3, 1) * f32(stats[3]) + f32(stats[2])], dim=-1)
        M = residual_matrix(system, x, x if gt is None else gt.to(dtype), stats)
        if sigma is not None:
            M = M / (sigma.to(dtype).reshape(-1, 1, 1, 1) + 1.0)
        val = M.sum()
        (g,) = torch.autograd.grad(val, Dl)
    return val.detach(), g


def sample_weights(sigma):
    """The w array of mcedm_pde_train_loss for pde_loss_prop_t: sum_i 1 / (sigma_i + 1), the same for every sample."""
    s = sigma.reshape(-1).to(torch.float32)
    return (1.0 / (s + 1.0)).sum().expand(s.numel()).contiguous()


# ---- module level: PlCondEdm on the ADM U-Net at the shapes of the cond_edm training golden (B = 3, 32 x 32) -------------------
# tag -> system, use_gt_pde, pde_loss_prop_t, the cond_p draw (>= cond_p = 0.8 switches the conditioning off)
MODULE_CASES = {"swe_self": ("swe_per", False, False, 0.1), "swe_gt": ("swe_per", True, False, 0.1),
                "swe_propt": ("swe_per", False, True, 0.1), "darcy": ("darcy", False, False, 0.1),
                "swe_nocond": ("swe_per", False, False, 0.9)}
# small tensors from both ends and the middle of the network; every other parameter is covered by its squared norm
MODULE_GRAD_NAMES = ["enc.128x128_conv.weight", "out_conv.weight", "dec.64x64_block1.conv1.bias", "enc.32x32_down.norm0.weight",
                     "map_layer1.bias"]
COND_P = 0.8                                   # hparams.model.cond_p of the module cases: below 1, so that the draw can drop the conditioning
OPT_DRAWS = (0.1, 0.9)                         # the cond_p draws of the two optimiser steps


def module_inputs(system):
    """(h, u, noise, rnd_normal, normaliser statistics): the inputs of the cond_edm training golden; for Darcy scaled so that the
    coefficient a = h stays positive under NORM_STATS."""
    h, u, noise, rnd_normal = fx.cond_training_inputs()
    if system == "darcy":
        return h * 0.25 + 1.05, u * 0.2, noise, rnd_normal, NORM_STATS
    return h, u, noise, rnd_normal, fx.TRAIN_NORM_STATS
MODULE_SEED = 13
