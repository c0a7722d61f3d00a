"""What tools/make_golden_ddpm_edm.py (the reference's runs, CPU) and the tests of PlCondEdm on the DDPM U-Net share: the
configuration (configs/model/edm_cond_h_res32.yaml at 32 x 32: ``name: edm_cond_h``, ``cat_cond: True``, ``self_cond: False``), the
parameter table with the widened conv_in, the tagged parameters and inputs, the sampler cases.  Everything here is regenerated
from tags; only the reference's outputs live in tests/golden/ddpm_edm*.npz."""
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import ddpm_oracle as ddo  # noqa: E402
from oracle import fixtures as fx  # noqa: E402

CFG = ddo.DdpmConfig(in_channels=1, out_ch=1, resolution=32, self_cond=False)
SEED = 31
B, H, W = 3, 32, 32
T_FWD = (math.log(0.05) / 4, 0.0, math.log(40.0) / 4)      # c_noise = ln(sigma) / 4 of three sigmas; the first is negative
SIGMAS = (0.05, 1.3, 40.0)                                 # get_denoised: three noise levels across the schedule
EDM_STEPS, EDM_CHURN = 18, 15.0
EVAL_N = 2
GUIDED_SYSTEM = "swe_per"


def param_shapes(cond_channels):
    """Model.state_dict() order with cat_cond: no cond_enc / combine_enc, conv_in reads cond_channels + in_channels planes."""
    return [(n, (s[0], cond_channels + CFG.in_channels, 3, 3) if n == "conv_in.weight" else s) for n, s in ddo.param_shapes(CFG)]


def make_params(cond_channels):
    """ddpm_oracle.make_params for every tensor but conv_in.weight, which is a tagged draw of the widened shape (same fill rule)."""
    P = ddo.make_params(CFG, SEED)
    shape = dict(param_shapes(cond_channels))["conv_in.weight"]
    u = fx.uniform(f"ddpme/P{cond_channels}/conv_in.weight", *shape)
    P["conv_in.weight"] = torch.from_numpy(ddo.fill_param("conv_in.weight", shape, u).astype(np.float32))
    return {n: P[n] for n, _ in param_shapes(cond_channels)}


def sampler_dict(**over):
    d = dict(name="edm", type="edm", timesteps=EDM_STEPS, sigma_min=0.002, sigma_max=80, rho=7, S_churn=EDM_CHURN, S_min=0,
             S_max="inf", S_noise=1, n_samples=1, n_repeat=2, n_time_h=128, n_time_u=0, return_last=True, select_by_pde=False,
             use_gt_pde_select=True, guide_dx=False, w=0.0, plot_scaled=False)
    d.update(over)
    return d


def hparams_dict(sampler=None, node_type=False, **model):
    """configs/model/edm_cond_h_res32.yaml with resolution 32 (a plain nested dict: each side wraps it in its own attribute dict)."""
    m = dict(type="simple", in_channels=1, cond_channels=1, cat_cond=True, out_ch=1, ch=CFG.ch, ch_mult=list(CFG.ch_mult),
             num_res_blocks=CFG.num_res_blocks, attn_resolutions=list(CFG.attn_resolutions), dropout=0.0, var_type="fixedsmall",
             ema_rate=0.999, ema=True, resamp_with_conv=True, resolution=CFG.resolution, self_cond=False, cond_p=1.0,
             dx_cond=False, cat_dx=False, dx_norm="l2", dx_detach=False, node_type=node_type)
    m.update(model)
    return dict(
        name="edm_cond_h", model=m,
        data=dict(normalization="gauss", uniform_dequantization=False, gaussian_dequantization=False, rescaled=False),
        diffusion=dict(beta_schedule="linear", beta_start=0.0001, beta_end=0.02, num_diffusion_timesteps=1000),
        optimization=dict(optimizer="Adam", lr=0.0002, weight_decay=0.0, beta1=0.9, amsgrad=False, eps=1e-8, grad_clip=1.0, loss="l2",
                          pde_loss_lambda=0.0, pde_loss_prop_t=False, use_gt_pde=False, factor=0.3, step_size=50),
        sampler=sampler or sampler_dict())


def fill(module, cond_channels, stats):
    """Tagged parameters into model and EMA copy, normaliser statistics (on the parameters' device)."""
    P = make_params(cond_channels)
    with torch.no_grad():
        for net in (module.model, module.ema_model.ma_model):
            named = list(net.named_parameters())
            assert [(n, tuple(p.shape)) for n, p in named] == [(n, tuple(s)) for n, s in param_shapes(cond_channels)]
            for n, p in named:
                p.copy_(P[n])
    dev = next(module.model.parameters()).device
    module.normalizer_input.set_stats(torch.tensor(stats[0]).to(dev), torch.tensor(stats[1]).to(dev))
    module.normalizer_target.set_stats(torch.tensor(stats[2]).to(dev), torch.tensor(stats[3]).to(dev))
    return module


def fwd_inputs(cond_channels):
    """x, cond in NCHW."""
    return fx.randn("ddpme/fwd/x", B, 1, H, W), fx.randn(f"ddpme/fwd/cond{cond_channels}", B, cond_channels, H, W)


def den_input():
    return fx.randn("ddpme/den/x", B, 1, H, W)


def sample_inputs():
    """h, u_noise in the reference's 'b h w c' layout."""
    return fx.randn("ddpme/smp/h", B, H, W, 1), fx.randn("ddpme/smp/u_noise", B, H, W, 1)


def guided_inputs():
    """h, u_noise of the guided case: small fields, so that the un-normalised h (STEP_NORM_STATS) stays positive."""
    return fx.randn("ddpme/gd/h", B, H, W, 1), fx.randn("ddpme/gd/u_noise", B, H, W, 1)


def edm_draws(tag, n, batch=B):
    """Step i's randn_like(x_cur) of models/ddim.py:1568, fp64 NCHW."""
    return [fx.randn(f"ddpme/{tag}/step{i}", batch, 1, H, W, dtype="float64") for i in range(n)]


def eval_inputs(which, n):
    """Un-normalised h, u 'b t x 1' and the injected randn_like '(n b) t x 1' of an evaluation step."""
    st = fx.STEP_NORM_STATS
    h = fx.randn(f"ddpme/{which}/h", fx.EVAL_B, H, W, 1) * st[1] + st[0]
    u = fx.randn(f"ddpme/{which}/u", fx.EVAL_B, H, W, 1) * st[3] + st[2]
    return h, u, fx.randn(f"ddpme/{which}/init", n * fx.EVAL_B, H, W, 1)


def bars_apart(a, b):
    """|a - b| in units of the comparison bar for reference b (rtol 1e-4, atol 1e-5 max|b|), per entry."""
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return (a - b).abs() / (1e-5 * float(b.abs().max()) + 1e-4 * b.abs())
