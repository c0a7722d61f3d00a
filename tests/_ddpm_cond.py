"""What tools/make_golden_ddpm_cond.py (the reference's runs, CPU) and the tests of PlCondDdim on the DDPM U-Net share: the
configuration (configs/model/ddim_cond_h_res32.yaml at 32 x 32), the parameter table with the cond_enc / combine_enc head, the
tagged parameters and inputs, the sampler cases.  Everything here is regenerated from tags; only the reference's outputs live in
tests/golden/ddpm_cond*.npz."""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import ddpm_oracle as ddo  # noqa: E402
from oracle import fixtures as fx  # noqa: E402

CFG = ddo.DdpmConfig(in_channels=1, out_ch=1, resolution=32, self_cond=True)
SEED = 29
B, H, W = 3, 32, 32
T_FWD = (0.0, 500.0, 999.0)
SIGMAS = (0.05, 1.3, 40.0)                      # get_denoised: three noise levels across the schedule
EDM_STEPS, EDM_CHURN = 18, 15.0
# tag -> (timesteps, skip_type, eta, w): the four cases of tests/golden/cond_ddim_sample.npz
DDIM_CASES = {"uni": (10, "uniform", 0.0, 0.0), "cfg_eta": (10, "uniform", 0.5, 0.5), "quad": (8, "quad", 0.0, 0.0),
              "uneven": (7, "uniform", 0.0, 0.0)}
DDIM_STEPS = {"uni": 10, "cfg_eta": 10, "quad": 8, "uneven": 8}       # 1000 // 7 = 142 walks 8 timesteps
EVAL_DDIM_STEPS, EVAL_N = 4, 2


def head_shapes(cond_channels, ch=CFG.ch):
    """cond_enc / combine_enc as Model registers them behind conv_in (models/ddim_blocks.py:279-306)."""
    return ddo.head_shapes(ch, cond_channels)


def param_shapes(cond_channels):
    base = ddo.param_shapes(CFG)
    at = [n for n, _ in base].index("conv_in.bias") + 1
    return base[:at] + head_shapes(cond_channels) + base[at:]


def make_params(cond_channels):
    """ddpm_oracle.make_params for the table without the head; tagged draws, same fill rule, for the head."""
    P = ddo.make_params(CFG, SEED)
    for name, shape in head_shapes(cond_channels):
        u = fx.uniform(f"ddpmc/P{cond_channels}/{name}", *shape)
        P[name] = torch.from_numpy(ddo.fill_param(name, shape, u).astype(np.float32))
    return {n: P[n] for n, _ in param_shapes(cond_channels)}


def sampler_dict(**over):
    d = dict(name="edm", type="edm", timesteps=EDM_STEPS, sigma_min=0.002, sigma_max=80, rho=7, S_churn=EDM_CHURN, S_min=0,
             S_max="inf", S_noise=1, n_samples=1, n_repeat=2, n_time_h=128, n_time_u=0, return_last=True, select_by_pde=False,
             use_gt_pde_select=True, guide_dx=False, w=0.0, plot_scaled=False, skip_type="uniform", eta=0.0)
    d.update(over)
    return d


def ddim_sampler(timesteps, skip_type="uniform", eta=0.0, w=0.0, **over):
    return sampler_dict(name="ddim", type="ddim", timesteps=timesteps, skip_type=skip_type, eta=eta, w=w, **over)


def hparams_dict(sampler=None, node_type=False):
    """configs/model/ddim_cond_h_res32.yaml with resolution 32 (a plain nested dict: each side wraps it in its own attribute dict)."""
    return dict(
        name="ddim_cond_h",
        model=dict(type="simple", in_channels=1, cond_channels=1, cat_cond=False, out_ch=1, ch=CFG.ch, ch_mult=list(CFG.ch_mult),
                   num_res_blocks=CFG.num_res_blocks, attn_resolutions=list(CFG.attn_resolutions), dropout=0.0, var_type="fixedsmall",
                   ema_rate=0.999, ema=True, resamp_with_conv=True, resolution=CFG.resolution, self_cond=True, cond_p=1.0,
                   dx_cond=False, cat_dx=False, dx_norm="l2", dx_detach=False, node_type=node_type),
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
    """x, cond, x_self_cond in NCHW."""
    return (fx.randn("ddpmc/fwd/x", B, 1, H, W), fx.randn(f"ddpmc/fwd/cond{cond_channels}", B, cond_channels, H, W),
            fx.randn("ddpmc/fwd/xsc", B, 1, H, W))


def sample_inputs():
    """h, u_noise in the reference's 'b h w c' layout."""
    return fx.randn("ddpmc/smp/h", B, H, W, 1), fx.randn("ddpmc/smp/u_noise", B, H, W, 1)


def edm_draws(tag, n, batch=B):
    """Step i's randn_like(x_cur) of models/ddim.py:1567, fp64 NCHW."""
    return [fx.randn(f"ddpmc/{tag}/step{i}", batch, 1, H, W, dtype="float64") for i in range(n)]


def eta_draw(tag, k, batch=B):
    """Step k's torch.rand_like(x) of models/ddim.py:1512: a tagged uniform in [0, 1), fp32."""
    return torch.from_numpy(((fx.uniform(f"ddpmc/ddim/{tag}/eta{k}", batch, 1, H, W) + 1.0) * 0.5).astype(np.float32))


def eval_inputs(which, n):
    """Un-normalised h, u 'b t x 1' and the injected randn_like '(n b) t x 1' of an evaluation step."""
    st = fx.STEP_NORM_STATS
    h = fx.randn(f"ddpmc/{which}/h", fx.EVAL_B, H, W, 1) * st[1] + st[0]
    u = fx.randn(f"ddpmc/{which}/u", fx.EVAL_B, H, W, 1) * st[3] + st[2]
    return h, u, fx.randn(f"ddpmc/{which}/init", n * fx.EVAL_B, H, W, 1)


def bars_apart(a, b):
    """|a - b| in units of the comparison bar for reference b (rtol 1e-4, atol 1e-5 max|b|), per entry."""
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return (a - b).abs() / (1e-5 * float(b.abs().max()) + 1e-4 * b.abs())


def check_cond_map(got, P, cond, what):
    """The map kernel's output against M = (Wc cond_enc.2) (*)circ GELU(cond_enc.0(cond)) + (Wx b_in + Wc b_enc2 + b_comb), everything
    in fp64 on the host (P: the parameters in fp64); the border ring (where the wrap-around is read), the four corners (both axes
    wrap) and the interior are held to the bar apart."""
    got = got.detach().cpu().double()
    ch = P["combine_enc.bias"].numel()
    Bc, _, R, _ = cond.shape
    Wx, Wc = P["combine_enc.weight"][:, :ch, 0, 0], P["combine_enc.weight"][:, ch:, 0, 0]
    g = F.gelu(F.conv2d(cond.double(), P["cond_enc.0.weight"], P["cond_enc.0.bias"]))
    w2 = torch.einsum("om,mckl->ockl", Wc, P["cond_enc.2.weight"])
    bias = Wx @ P["conv_in.bias"] + Wc @ P["cond_enc.2.bias"] + P["combine_enc.bias"]
    ref = F.conv2d(F.pad(g, (1, 1, 1, 1), mode="circular"), w2, bias)
    assert got.shape == ref.shape == (Bc, ch, R, R)
    ring = torch.ones(R, R, dtype=torch.bool)
    ring[1:-1, 1:-1] = False
    corners = torch.zeros(R, R, dtype=torch.bool)
    corners[0, 0] = corners[0, -1] = corners[-1, 0] = corners[-1, -1] = True
    atol = 1e-5 * float(ref.abs().max())
    for where, sel in (("interior", ~ring), ("border ring", ring & ~corners), ("corners", corners)):
        err, lim = (got[..., sel] - ref[..., sel]).abs(), atol + 1e-4 * ref[..., sel].abs()
        print(f"cond_map {what} {where}: worst err / bar {float((err / lim).max()):.4f}")
        assert bool((err <= lim).all()), (where, float(err.max()))
    # zero padding in place of circular would miss the ring by far more than the bar
    zp = F.conv2d(g, w2, bias, padding=1)
    assert float((bars_apart(zp[..., ring], ref[..., ring]) >= 100).double().mean()) > 0.5
