"""What tools/make_golden_cond_guided.py (the reference's guided runs, CPU) and the tests of PlCondDdim's PDE guidance (guide_dx,
models/ddim.py:1499-1503 and 1576-1590) share: the cases, the sampler blocks, the tagged inputs and draws, the comparison bar and
the fp64 formula of one guided DDIM step.  Everything here is regenerated from tags; only the reference's outputs live in
tests/golden/cond_guided.npz (ADM U-Net) and cond_guided_ddpm.npz (DDPM U-Net)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import fixtures as fx  # noqa: E402
from tests import _ddpm_cond as D  # noqa: E402

B, H, W = 3, 32, 32
NETS = ("adm", "ddpm")
GOLDEN = {"adm": "cond_guided.npz", "ddpm": "cond_guided_ddpm.npz"}      # one file per network, each under 1 MB
WEIGHT = 5.0                                   # `weight = 5.` of models/ddim.py:1502, 1577
# tag -> (sampler method, PDE system, sampler-block settings on top of D.sampler_dict)
CASES = {
    "ddim": ("sample", "swe_per", dict(type="ddim", name="ddim", timesteps=5, skip_type="uniform", eta=0.0, w=0.0)),
    "ddim_cfg_eta": ("sample", "swe_per", dict(type="ddim", name="ddim", timesteps=5, skip_type="uniform", eta=0.5, w=0.5)),
    "vp": ("sample_edm", "swe_per", dict(timesteps=6, sigma_max=5.0, S_churn=0.0, w=0.0)),
    "vp_churn_cfg": ("sample_edm", "swe_per", dict(timesteps=6, sigma_max=5.0, S_churn=15.0, w=0.5)),
    "darcy": ("sample", "darcy", dict(type="ddim", name="ddim", timesteps=5, skip_type="uniform", eta=0.0, w=0.0)),
}
STEPS = {"ddim": 5, "ddim_cfg_eta": 5, "vp": 6, "vp_churn_cfg": 6, "darcy": 5}      # 1000 // 5 = 200 walks 5 timesteps
MIN_SLOTS = 4                                  # the compared prefix covers at least 4 steps


def cases_of(net):
    return [t for t in CASES if not (t == "darcy" and net != "adm")]


def sampler_dict(tag, guide_dx=True, **over):
    d = D.sampler_dict(guide_dx=guide_dx, **CASES[tag][2])
    d.update(over)
    return d


def inputs(scale=1.0):
    """h, u_noise in the reference's 'b h w c' layout; scale: the perturbation of the generator's rerun."""
    return fx.randn("cguided/h", B, H, W, 1) * 0.3, fx.randn("cguided/u_noise", B, H, W, 1) * scale


def eta_draw(tag, k):
    """Step k's torch.rand_like(x) of models/ddim.py:1512: a tagged uniform in [0, 1), fp32."""
    return torch.from_numpy(((fx.uniform(f"cguided/{tag}/eta{k}", B, 1, H, W) + 1.0) * 0.5).astype(np.float32))


def step_draws(tag):
    """Step i's randn_like(x_cur) of models/ddim.py:1568, fp64 NCHW."""
    return [fx.randn(f"cguided/{tag}/step{i}", B, 1, H, W, dtype="float64") for i in range(STEPS[tag])]


def bar(ref):
    """tests/_tol.close_per_entry's bar for one slot of reference `ref`, per entry."""
    ref = torch.as_tensor(ref).double()
    return 1e-5 * float(ref.abs().max()) + 1e-4 * ref.abs()


def bars_apart(a, b):
    """max |a - b| / bar(b) over one slot."""
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float(((a - b).abs() / bar(b)).max())


def ddim_step_fp64(xt, F, Fu, nz, dx, w, gw, s0, s1, sa, c1, c2):
    """One step of PlCondDdim.sample with guidance in fp64 from the fp32 inputs (:1497-1515): returns x0, xt_next and the
    magnitude `mag` of et's terms, |w1 F| + |w Fu| + |gw dx| (Fu, nz, dx: None when absent)."""
    x, F = xt.double(), F.double()
    w1f, wf = float(np.float32(w + 1.0)), float(np.float32(w))
    et = w1f * F - wf * Fu.double() if Fu is not None else F
    mag = (w1f * F).abs() + (wf * Fu.double()).abs() if Fu is not None else F.abs()
    if dx is not None:
        g = gw * dx.double()
        et, mag = et - g, mag + g.abs()
    x0 = (x - et * s1) / s0
    xn = sa * x0 + (c1 * nz.double() if nz is not None else 0.0) + c2 * et
    return x0, xn, mag
