"""What tests/test_sampler_exact_cpu.py and tests/test_hip_sampler_exact.py share: networks that return a constant, the cases'
schedules and inputs, the CPU reference loops and the bit comparison.  No GPU import here.

With every parameter zero except the bias of the last convolution, either U-Net returns that bias and nothing else (each
GroupNorm sees a zero-variance tensor and maps it to its zero bias, every convolution adds its zero bias to a zero sum).  A
sampler around such a network is a closed-form recurrence in the reference's own fp32 / fp64 arithmetic, and the oracle's
loops evaluate that recurrence on the CPU without any network noise floor: the device must reproduce it bit for bit."""
import contextlib
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
from oracle import mcedm_oracle as orc  # noqa: E402

# one distinct value per output channel, none of them representable in fp32
BIAS = (0.37, -1.21)
B, H, W = 3, 8, 12                                  # the ADM cases: H != W, both multiples of 4 (three levels)
BIG = (5, 232, 228)                                 # 5 * 2 * 232 * 228 = 528,960 state elements > the 2048 x 256 threads of grid_for
SIGMA_DATA = 0.5
# a guidance weight for which fl32(fl32(w) + 1) is not fl32(w + 1), the factor (w + 1) * F of the reference's Python scalar
W_ODD = 0.32
# timesteps 6, rho 5 gives sigmas 80, 30.39, 9.14, 1.88, 0.182, 0.002: the window [0.05, 30] churns steps 2, 3 and 4 only
WINDOW = dict(timesteps=6, rho=5.0, S_min=0.05, S_max=30.0, S_churn=15.0, S_noise=1.007)
WINDOW_CHURNS = [False, False, True, True, True, False]

# the schedules the single-task samplers are handed as arrays.  VP (vp_schedule): sigmas and t_hat wishes (None = the step does
# not churn), each rounded onto the DDPM table.  EDM (edm_schedule): sigmas used as they are, t_hat = t + gamma t inside a window
VP_SIGMAS = ([20.0, 5.0, 1.0, 0.1], [None, 6.0, None, 0.12])
VP_GUIDED_SIGMAS = ([2.0, 1.0, 0.3, 0.05], [None, 1.2, None, None])      # tame states: the residual gradient stays finite
ONE_STEP = ([5.0], [6.0])                           # timesteps == 1: Euler only
EDM_SCHED = dict(sigmas=[20.0, 5.0, 1.0, 0.1], S_churn=15.0, S_min=0.5, S_max=10.0)      # steps 1 and 2 churn
EDM_ONE_STEP = dict(sigmas=[5.0], S_churn=15.0, S_min=0.5, S_max=10.0)
# RePaint on the DDPM table (sigma_min becomes the table's 0.01): sigmas 80.3, 32.1, 10.5, 2.49, 0.325, 0.01 -- steps 2, 3, 4 churn
REPAINT = dict(timesteps=6, rho=5.0, S_min=0.05, S_max=30.0, S_churn=15.0, S_noise=1.007, n_repeat=3, n_time_h=3, n_time_u=5)
DDIM_REPAINT = dict(timesteps=4, skip_type="uniform", eta=0.5, n_repeat=2, n_time_h=3, n_time_u=5)

CFG_JOINT = fx.CFG_P                                                   # in 2, cond 2: the masked sampler
CFG_SINGLE = fx.CFG_C                                                  # in 1, cond 1: the unmasked sampler, SWE guidance
CFG_WIDE = orc.UNetConfig(in_channels=1, cond_channels=2, out_ch=1)    # PlCondDdim: cond' = cat(h, x_self_cond)

# the DDPM U-Net at 8 x 8 with one level, the smallest member the architecture tests run (tests/_ddpm_arch.py "one", "cat_one2")
R = 8
_ONE = dict(ch=64, ch_mult=(1,), num_res_blocks=1, attn_resolutions=(8,), resolution=R)
CFG_D_JOINT = ddo.DdpmConfig(in_channels=2, out_ch=2, self_cond=True, **_ONE)                                     # PlDdim
CFG_D_HEAD = ddo.DdpmConfig(in_channels=1, out_ch=1, self_cond=True, cond_channels=1, **_ONE)                     # PlCondDdim
CFG_D_CAT = ddo.DdpmConfig(in_channels=1, out_ch=1, self_cond=False, cond_channels=1, cat_cond=True, **_ONE)      # PlCondEdm


# ---- constant networks ----------------------------------------------------------------------------------------------------
def constant_params(make_params, cfg, bias):
    """``make_params(cfg)``'s table with every parameter zero and the bias of the last convolution (out_conv.bias on the ADM
    U-Net, conv_out.bias on the DDPM U-Net) set to ``bias``, one value per output channel."""
    P = {k: torch.zeros_like(v) for k, v in make_params(cfg).items()}
    last = [k for k in ("out_conv.bias", "conv_out.bias") if k in P]
    assert len(last) == 1, last
    b = torch.tensor(list(bias), dtype=torch.float32)
    assert b.shape == P[last[0]].shape, (b.shape, P[last[0]].shape)
    P[last[0]] = b
    return P


def bias_of(cfg, zero=False):
    n = cfg.out_ch
    return (0.0,) * n if zero else BIAS[:n]


def const_net(bias):
    """``net(x, labels, *conditioning) -> F`` that returns the bias without running a network: what
    tests/test_sampler_exact_cpu.py shows both U-Nets to compute on constant_params."""
    b = torch.tensor(list(bias), dtype=torch.float32).view(1, -1, 1, 1)

    def net(x, *a, **k):
        return b.expand(x.shape[0], -1, x.shape[2], x.shape[3]).contiguous()
    return net


def adm_net(P, cfg):
    """The ADM U-Net in get_denoised's calling convention."""
    return lambda x, labels, c, dx=None: orc.unet_forward(P, cfg, x, labels, c, dx=dx)


def ddpm_net(P, cfg):
    """The DDPM U-Net as ``net(x, labels, cond, x_self_cond)``."""
    return lambda x, labels, cond=None, x_self_cond=None: ddo.model_forward(P, cfg, x, labels, x_self_cond=x_self_cond, cond=cond)


def ddpm_cat_net(P, cfg):
    """The cat_cond DDPM U-Net in get_denoised's calling convention (PlCondEdm on Model)."""
    return lambda x, labels, c, dx=None: ddo.model_forward(P, cfg, x, labels, cond=c)


# ---- schedules ------------------------------------------------------------------------------------------------------------
def churns(t_steps, S_churn, S_min, S_max):
    """Per step: does gamma > 0 hold (mcedm.py:606)."""
    return [S_churn > 0 and S_min <= float(t) <= S_max for t in list(t_steps)[:-1]]


def within_ulps(a, b, n=2):
    """Every entry of the float64 sequences within n ulp of the other's."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all(np.abs(a - b) <= n * np.spacing(np.maximum(np.abs(a), np.abs(b)))))


def ddpm_tables(cfg=CFG_D_JOINT):
    """(edm_steps, alphas_cumprod_ext) as the library is handed them.  Under ieee_sqrt: sample_edm_repaint rebuilds the sigma
    table itself, and inside that context it must arrive at the entries the library was given."""
    betas = ddo.betas_of(cfg)
    with ieee_sqrt():
        return ddo.edm_steps_of(betas), ddo.alphas_ext_of(betas)


def vp_schedule(steps_table, sigmas, hats, num_timesteps=1000):
    """(t_steps [N + 1], t_hat [N], c_noise [2 N]) of PlCondDdim.sample_edm from wished-for sigmas: each rounded onto the
    table (round_sigma), the labels num_timesteps - 1 - index at t_hat[i] and at t_steps[i + 1] (0 behind the last step)."""
    rs = lambda v: float(ddo.round_sigma(steps_table, torch.tensor([v], dtype=torch.float64))[0])      # noqa: E731
    cn = lambda v: float(num_timesteps - 1 - int(ddo.round_sigma(steps_table, torch.tensor([v], dtype=torch.float32), return_index=True)[0]))      # noqa: E731
    t = [rs(s) for s in sigmas] + [0.0]
    th = [t[i] if hats[i] is None else rs(hats[i]) for i in range(len(sigmas))]
    assert all(th[i] >= t[i] for i in range(len(sigmas)))
    c = []
    for i in range(len(sigmas)):
        c += [cn(th[i]), cn(t[i + 1]) if i < len(sigmas) - 1 else 0.0]
    return t, th, c


def edm_schedule(sigmas, S_churn, S_min, S_max):
    """The same triple for PlCondEdm.sample_edm, whose round_sigma is the identity: t_hat = t_cur + gamma t_cur in float64
    (models/ddim.py:1566-1567), c_noise = ln(sigma) / 4 in fp32."""
    cn = lambda v: float(torch.tensor(v, dtype=torch.float32).log() / 4)      # noqa: E731
    N = len(sigmas)
    t = [float(s) for s in sigmas] + [0.0]
    th = []
    for i in range(N):
        gamma = min(S_churn / N, math.sqrt(2) - 1) if S_min <= t[i] <= S_max else 0
        th.append(t[i] + gamma * t[i])
    c = []
    for i in range(len(sigmas)):
        c += [cn(th[i]), cn(t[i + 1]) if i < len(sigmas) - 1 else 0.0]
    return t, th, c


# ---- inputs ---------------------------------------------------------------------------------------------------------------
def fractional_mask(tag, shape):
    """1 = missing, with 0 / 0.75 / 1 entries in every channel of every sample."""
    u = torch.from_numpy(fx.uniform(f"exact/{tag}/mask", *shape))
    return torch.where(u < -1 / 3, 0.0, torch.where(u < 1 / 3, 0.75, 1.0)).to(torch.float32)


def draws64(tag, n, shape):
    """n fp64 normal draws with all 53 bits in use (nothing about them is fp32-representable)."""
    return [fx.randn(f"exact/{tag}/step{i}", *shape, dtype=np.float64) for i in range(n)]


def uniform32(tag, n, shape):
    """n uniform fp32 draws in [0, 1): the torch.rand_like of the DDIM samplers."""
    return [torch.from_numpy(((fx.uniform(f"exact/{tag}/eta{i}", *shape) + 1.0) * 0.5).astype(np.float32)) for i in range(n)]


# ---- a square root that is the same function on every host ----------------------------------------------------------------
@contextlib.contextmanager
def ieee_sqrt():
    """Inside this context Tensor.sqrt / torch.sqrt of a CPU float tensor is numpy's, i.e. the correctly rounded one.

    torch's own CPU square root goes through a vector math library and is neither correctly rounded nor the same function on
    every host: of 400,000 fp32 values 0.6 % differ from the IEEE result on one x86 host and 18 % on another (measured; numpy:
    0 on both, division, products and conversions: 0 on both).  The square roots of the sampler loops -- sqrt(sigma^2 + sd^2),
    sqrt(alpha), sqrt(1 - alpha), sqrt(t_hat^2 - t_cur^2) -- are correctly rounded in the kernels and in the host code of the
    library (IEEE sqrtf / sqrt), as they are where the reference itself samples on a device.  A bit-for-bit reference has to take
    the one well-defined value, so the oracle's loops run unchanged under this context."""
    real_method, real_fn = torch.Tensor.sqrt, torch.sqrt

    def wrap(real):
        def sqrt(self, *a, **k):
            if a or k or self.device.type != "cpu" or self.dtype not in (torch.float32, torch.float64) or self.requires_grad:
                return real(self, *a, **k)
            return torch.from_numpy(np.asarray(np.sqrt(self.numpy()))).reshape(self.shape)
        return sqrt
    torch.Tensor.sqrt, torch.sqrt = wrap(real_method), wrap(real_fn)
    try:
        yield
    finally:
        torch.Tensor.sqrt, torch.sqrt = real_method, real_fn


# ---- comparison -----------------------------------------------------------------------------------------------------------
def ulps_apart(got, ref):
    """The largest distance between corresponding entries, counted in representable numbers of their common dtype."""
    got, ref = torch.as_tensor(got), torch.as_tensor(ref)
    assert got.dtype == ref.dtype and got.shape == ref.shape, (got.dtype, ref.dtype, got.shape, ref.shape)
    it = torch.int64 if got.dtype == torch.float64 else torch.int32
    lo = torch.iinfo(it).min

    def ordered(v):                      # sign-magnitude bits -> an integer that grows with the value
        i = v.contiguous().view(it).to(torch.int64)
        return torch.where(i < 0, lo - i, i)
    if not bool(torch.isfinite(got).all()):
        return math.inf
    return int((ordered(got) - ordered(ref)).abs().max()) if got.numel() else 0


def check_exact(what, got, ref):
    """torch.equal(got, ref), with the largest difference printed in ulps of the output dtype first."""
    got = torch.as_tensor(got).detach().cpu()
    assert got.dtype == ref.dtype and got.shape == ref.shape, (what, got.dtype, ref.dtype, got.shape, ref.shape)
    d = ulps_apart(got, ref)
    print(f"{what}: max difference {d} ulp ({str(got.dtype).split('.')[-1]}), max|ref| {float(ref.abs().max()):.4g}")
    if not torch.equal(got, ref):
        bad = (got != ref) | torch.isnan(got)
        first = [int(v) for v in bad.nonzero()[0]]
        raise AssertionError(f"{what}: {int(bad.sum())} of {got.numel()} entries differ, by up to {d} ulp; first at {first}: "
                             f"got {got[tuple(first)].item()!r}, reference {ref[tuple(first)].item()!r}")
