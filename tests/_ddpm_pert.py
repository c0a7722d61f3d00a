"""What tools/make_golden_ddpm_pert.py (the reference's ``Model``, CPU) and the tests of the per-sample-timestep entries of the
DDPM U-Net share.  Networks, parameters and inputs are those of tests/_ddpm_arch.py (B = 2); only the reference's outputs live
in tests/golden/ddpm_pert.npz: every row of ``_ddpm_arch.ALL`` at t = (3, 937) and at t = (937, 3), with x_self_cond and cond
given wherever the network takes them."""
import math

import torch

from tests import _ddpm_arch as A

B = A.B
T_PAIRS = ((3.0, 937.0), (937.0, 3.0))       # an early and a late timestep in one batch, and the two swapped
T_ROWS = (0.0, 3.0, 937.0, 999.0, -0.7489)   # the ends of the DDPM range, the pair above, and an EDM label ln(0.05) / 4
T_FIVE = (0.0, 999.0, 3.0, 937.0, 500.0)
SIGMAS = (0.05, 3.0)                         # EDM noise levels either side of sigma_data
SIGMA_DATA = 1.0


def key(tag, ts):
    return f"{tag}::t{int(ts[0])}_{int(ts[1])}"


def oracle_forward(tag, P, ts, sample=None):
    """ddpm_oracle.model_forward at one timestep per sample; x_self_cond and cond given where the network takes them."""
    x, xsc, cond = A.inputs(tag)
    with torch.no_grad():
        return A.ddo.model_forward(P, A.ALL[tag], x, torch.tensor(ts, dtype=torch.float32), x_self_cond=xsc, cond=cond)


def temb_rows64(tag, P64, ts):
    """[len(ts), rows] in fp64: row r = temb_proj_r . swish(MLP(emb(t))) + temb_proj.bias[r] + conv1.bias[r], the blocks in the
    order of the parameter table.  The embedding's arguments are the fp32 products t * freq of the fp32 frequency table (what
    ddpm_oracle.timestep_embedding describes): sin and cos of large arguments see every bit of them."""
    cfg = A.ALL[tag]
    freqs = A.ddo.timestep_freqs(cfg.ch)
    t = torch.tensor(ts, dtype=torch.float32)
    arg = (t[:, None] * freqs[None, :]).double()
    emb = torch.cat([arg.sin(), arg.cos()], dim=1)
    swish = lambda v: v * torch.sigmoid(v)
    e = swish(emb @ P64["temb.dense.0.weight"].T + P64["temb.dense.0.bias"])
    e = swish(e @ P64["temb.dense.1.weight"].T + P64["temb.dense.1.bias"])
    rows = []
    for name, _ in A.ddo.param_shapes(cfg):
        if name.endswith(".temb_proj.weight"):
            blk = name[:-len(".temb_proj.weight")]
            rows.append(e @ P64[name].T + P64[blk + ".temb_proj.bias"] + P64[blk + ".conv1.bias"])
    return torch.cat(rows, dim=1)


def edm_precond64(tag, P64, sigma, use_cond):
    """(D, F) of model_precond (models/ddim.py:1654-1666) in fp64 on a cat_cond row of _ddpm_arch: x is the row's input scaled to
    the noise level, sigma one level per sample.  c_noise is the fp32 value ln(sigma) / 4 the network is given in fp32 too."""
    x, _, cond = A.inputs(tag)
    sg32 = torch.tensor(sigma, dtype=torch.float32)
    x = edm_input(tag, sigma).double()
    sg = sg32.double().reshape(-1, 1, 1, 1)
    sd = SIGMA_DATA
    c_skip = sd ** 2 / (sg ** 2 + sd ** 2)
    c_out = sg * sd / (sg ** 2 + sd ** 2).sqrt()
    c_in = 1 / (sd ** 2 + sg ** 2).sqrt()
    c_noise = (sg32.log() / 4).double()
    with torch.no_grad():
        F = A.ddo.model_forward(P64, A.ALL[tag], c_in * x, c_noise, cond=cond.double() if use_cond else None)
    return c_skip * x + c_out * F, F


def edm_input(tag, sigma):
    """The row's x as a state at noise level sigma[b]: x * sqrt(sigma_b^2 + sigma_data^2), fp32."""
    x = A.inputs(tag)[0]
    return x * torch.tensor([math.sqrt(s * s + SIGMA_DATA ** 2) for s in sigma], dtype=torch.float32).reshape(-1, 1, 1, 1)


# ---- the noising pass of the three modules on the DDPM U-Net (tests/golden/ddpm_pert_steps.npz) ------------------------------------
# One small network per module: ch 64, ch_mult (1, 1), 16 x 16, attention at 8 x 8, B = 4.
#   ddim  PlDdim      joint (h, u) state, self-conditioning
#   cond  PlCondDdim  u given h through the cond_enc head, self-conditioning
#   edm   PlCondEdm   u given h concatenated to the input (cat_cond), no self-conditioning
from oracle import fixtures as fx  # noqa: E402
from tests import _ddpm_cond as DC  # noqa: E402

SB, SR = 4, 16
STEP_SEED = 43
T_HALF = (3, 998, 500)                       # the injected antithetic half (n // 2 + 1 = 3 draws): t = (3, 998, 500, 996)
COND_P = 0.8
STATS = fx.TRAIN_NORM_STATS
_BASE = dict(ch=64, ch_mult=(1, 1), num_res_blocks=1, attn_resolutions=(8,), resolution=SR)
STEP_CFG = {
    "ddim": A.ddo.DdpmConfig(in_channels=2, out_ch=2, self_cond=True, **_BASE),
    "cond": A.ddo.DdpmConfig(in_channels=1, out_ch=1, self_cond=True, cond_channels=1, **_BASE),
    "edm": A.ddo.DdpmConfig(in_channels=1, out_ch=1, self_cond=False, cond_channels=1, cat_cond=True, **_BASE),
}
# case -> the torch.rand draws the forward consumes, in the reference's order: the cond_p draw (conditioning on below 0.8), then,
# on a self-conditioning network, the draw of the pre-pass (taken below 0.5)
STEP_CASES = {
    "ddim": {"sc": (0.5, 0.2), "nosc": (0.5, 0.7)},                       # cond_p is 0 there: never conditioned
    "cond": {"cond_sc": (0.1, 0.2), "cond_nosc": (0.1, 0.7), "nocond_sc": (0.9, 0.2), "nocond_nosc": (0.9, 0.7)},
    "edm": {"cond": (0.1,), "nocond": (0.9,)},
}


def step_hparams(kind):
    cfg = STEP_CFG[kind]
    hp = DC.hparams_dict()
    hp["name"] = {"ddim": "ddim", "cond": "ddim_cond_h", "edm": "edm_cond_h"}[kind]
    hp["model"].update(in_channels=cfg.in_channels, out_ch=cfg.out_ch, cond_channels=cfg.cond_channels, cat_cond=cfg.cat_cond,
                       ch=cfg.ch, ch_mult=list(cfg.ch_mult), num_res_blocks=cfg.num_res_blocks,
                       attn_resolutions=list(cfg.attn_resolutions), resolution=cfg.resolution, self_cond=cfg.self_cond, cond_p=COND_P)
    return hp


def step_params(kind, dtype=torch.float32):
    return {k: v.to(dtype) for k, v in A.ddo.make_params(STEP_CFG[kind], STEP_SEED).items()}


def step_fill(module, kind):
    """The tagged parameters into the model and its EMA copy, the normaliser statistics (on the parameters' device)."""
    P = step_params(kind)
    with torch.no_grad():
        for net in (module.model, module.ema_model.ma_model):
            named = list(net.named_parameters())
            assert [n for n, _ in named] == list(P)
            for n, p in named:
                p.copy_(P[n])
    dev = next(module.model.parameters()).device
    module.normalizer_input.set_stats(torch.tensor(STATS[0]).to(dev), torch.tensor(STATS[1]).to(dev))
    module.normalizer_target.set_stats(torch.tensor(STATS[2]).to(dev), torch.tensor(STATS[3]).to(dev))
    module.h_ch = module.u_ch = 1
    return module


def step_batch():
    """Un-normalised h, u in the reference's 'b h w c' layout."""
    return fx.randn("ddpmp/step/h", SB, SR, SR, 1) * STATS[1] + STATS[0], fx.randn("ddpmp/step/u", SB, SR, SR, 1) * STATS[3] + STATS[2]


def step_draws(kind):
    """noise (randn_like of the state), the antithetic half of t, rnd_normal of the EDM sigma"""
    C = STEP_CFG[kind].in_channels
    return fx.randn(f"ddpmp/step/{kind}/noise", SB, C, SR, SR), torch.tensor(T_HALF), fx.randn("ddpmp/step/rnd_normal", SB, 1, 1, 1)


def step_t():
    half = torch.tensor(T_HALF)
    return torch.cat([half, 999 - half])[:SB]


def step_state(kind):
    """(x, cond) of the module's forward in NCHW fp32: the normalised target (ddim: the joint state) and the conditioning h."""
    h, u = step_batch()
    hn = ((h - STATS[0]) / STATS[1]).permute(0, 3, 1, 2).contiguous()
    un = ((u - STATS[2]) / STATS[3]).permute(0, 3, 1, 2).contiguous()
    return (torch.cat([hn, un], dim=1).contiguous(memory_format=torch.contiguous_format), None) if kind == "ddim" else (un, hn)


def step_forward64(kind, case, P64):
    """(output, x0_t, loss) of forward / training_step in fp64 on the fp32 inputs and draws: models/ddim.py:195-226 with
    NoiseEstimationLoss (mean over the batch of the per-sample sums) for ddim / cond, :1654-1694 with the EDM weight for edm."""
    cfg = STEP_CFG[kind]
    x, cond = step_state(kind)
    noise, _, rnd = step_draws(kind)
    x, noise = x.double(), noise.double()
    draws = list(STEP_CASES[kind][case])
    fwd = lambda xx, tt, **kw: A.ddo.model_forward(P64, cfg, xx, tt, **kw)
    with torch.no_grad():
        if kind == "edm":
            sigma32 = (rnd * 1.2 + (-1.2)).exp().reshape(-1)                      # fp32, as the module draws it
            sg = sigma32.double().reshape(-1, 1, 1, 1)
            xn = x + noise * sg
            c = cond.double() if draws.pop(0) < COND_P else None
            c_in, c_noise = 1 / (1.0 + sg ** 2).sqrt(), (sigma32.log() / 4).double()
            D = 1.0 / (sg ** 2 + 1.0) * xn + sg / (sg ** 2 + 1.0).sqrt() * fwd(c_in * xn, c_noise, cond=c)
            w = (sg ** 2 + 1.0) / sg ** 2
            return D, D, (w * (D - x) ** 2).sum(dim=(1, 2, 3)).mean()
        t = step_t()
        a = (1 - A.ddo.betas_of(cfg)).cumprod(dim=0).index_select(0, t).double().view(-1, 1, 1, 1)
        xn = x * a.sqrt() + noise * (1.0 - a).sqrt()
        r_cond = draws.pop(0)                                                     # PlDdim's cond_p is 0: never conditioned
        c = cond.double() if (kind == "cond" and r_cond < COND_P) else None
        x0 = lambda F: (xn - F * (1 - a).sqrt()) / a.sqrt()
        xsc = x0(fwd(xn, t.float(), cond=c)) if draws.pop(0) < 0.5 else None
        out = fwd(xn, t.float(), cond=c, x_self_cond=xsc)
        return out, x0(out), ((out - noise) ** 2).sum(dim=(1, 2, 3)).mean()
