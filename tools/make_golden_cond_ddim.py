"""Golden vectors for PlCondDdim on the ADM U-Net with self-conditioning (configs/model/adm_cond_h_res32.yaml at 32 x 32), made by
RUNNING THE REFERENCE's models/ddim.py PlCondDdim on the CPU with every random draw injected:

  * DhariwalUNet.forward with self_cond (x_self_cond given / None, labels t in {0, 1, 500, 999})
  * training_step: loss and gradients in the four branches (conditioning on / off) x (self-conditioning pre-pass on / off)
  * three optimiser steps (clip_grad_norm_ 1.0, torch.optim.Adam, EmaModel.update)
  * sample_edm: 50 steps, S_churn 15, w in {0, 0.5}

    python tools/make_golden_cond_ddim.py          # rewrites tests/golden/cond_ddim.npz (needs the reference checkout)
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import make_golden as mg            # noqa: E402  sets up the reference import and the Lightning stand-in

import torch                        # noqa: E402
from models.ddim import PlCondDdim  # noqa: E402  (reference)

from oracle import fixtures as fx   # noqa: E402
from oracle import mcedm_oracle as orc  # noqa: E402

SEED = 17
# the self-conditioning network's parameter table is the cat_cond one with the conditioning widened by in_channels
CFG = orc.UNetConfig(in_channels=1, cond_channels=2, out_ch=1)
B, H, W = 3, 32, 32
GRAD_NAMES = ["enc.128x128_conv.weight", "enc.128x128_conv.bias", "out_conv.weight", "dec.32x32_in0.qkv.weight",
              "map_layer0.weight", "map_layer1.bias", "enc.32x32_down.norm0.weight"]
BRANCHES = {"cond_sc": (0.1, 0.2), "cond_nosc": (0.1, 0.7), "nocond_sc": (0.9, 0.2), "nocond_nosc": (0.9, 0.7)}


def hparams(sampler):
    hp = mg.make_hparams(orc.UNetConfig(in_channels=1, cond_channels=1, out_ch=1), sampler)
    hp["name"] = "adm_cond_h"
    hp.model.update(type="simple", var_type="fixedsmall", node_type=False, self_cond=True, cond_p=0.8)
    hp["diffusion"] = mg._wrap(dict(beta_schedule="linear", beta_start=0.0001, beta_end=0.02, num_diffusion_timesteps=1000))
    return hp


def build(sampler=None):
    m = PlCondDdim(hparams(sampler or mg.sampler_dict()))
    assert [(n, tuple(p.shape)) for n, p in m.model.named_parameters()] == [(n, tuple(s)) for n, s in orc.param_shapes(CFG)]
    P = orc.make_params(CFG, SEED)
    with torch.no_grad():
        for n, p in m.model.named_parameters():
            p.copy_(P[n])
        for n, p in m.ema_model.ma_model.named_parameters():
            p.copy_(P[n])
    st = fx.TRAIN_NORM_STATS
    m.normalizer_input.set_stats(torch.tensor(st[0]), torch.tensor(st[1]))
    m.normalizer_target.set_stats(torch.tensor(st[2]), torch.tensor(st[3]))
    return m


def inputs():
    """Shared with tests/test_hip_cond_ddim.py (same tags)."""
    h = fx.randn("cddim/h", B, H, W, 1) * 0.2 + 1.4
    u = fx.randn("cddim/u", B, H, W, 1) * 0.5
    noise = fx.randn("cddim/noise", B, 1, H, W)
    t_half = torch.tensor([3, 998])                            # randint(0, 1000, (n // 2 + 1,))
    return h, u, noise, t_half


class _Draws:
    """torch.randint / torch.rand replaced by queues (the reference's draws in training_step / forward)."""

    def __init__(self, ints, rands):
        self.ints, self.rands = list(ints), list(rands)

    def __enter__(self):
        self._ri, self._r = torch.randint, torch.rand
        torch.randint = lambda *a, **k: self.ints.pop(0)
        torch.rand = lambda *a, **k: torch.tensor([self.rands.pop(0)])
        return self

    def __exit__(self, *a):
        torch.randint, torch.rand = self._ri, self._r


def main():
    out = {}
    # ---- forward with self-conditioning
    m = build()
    x = fx.randn("cddim/fwd/x", 4, 1, H, W)
    cond = fx.randn("cddim/fwd/cond", 4, 1, H, W)
    xsc = fx.randn("cddim/fwd/xsc", 4, 1, H, W)
    labels = torch.tensor([0.0, 1.0, 500.0, 999.0])
    with torch.no_grad():
        out["fwd_F_sc"] = m.model(x, labels, cond, x_self_cond=xsc)
        out["fwd_F_nosc"] = m.model(x, labels, cond)
        out["fwd_F_nocond"] = m.model(x, labels, None, x_self_cond=xsc)
    out["state_dict_keys"] = torch.tensor([0])
    keys = list(m.state_dict().keys())

    # ---- training step, four branches
    h, u, noise, t_half = inputs()
    for tag, (r_cond, r_sc) in BRANCHES.items():
        m = build()
        with mg._Inject([noise]), _Draws([t_half], [r_cond, r_sc]):
            loss = m.training_step((h, None, None, u), 0)
        loss.backward()
        grads = {n: p.grad for n, p in m.model.named_parameters()}
        out[f"{tag}::loss"] = loss.detach()
        for n in GRAD_NAMES:
            out[f"{tag}::grad::{n}"] = grads[n]
        out[f"{tag}::grad_sqnorm_each"] = torch.tensor([float((g.double() ** 2).sum()) for g in grads.values()])

    # ---- three optimiser steps (Lightning: closure, clip_grad_norm_(1.0), Adam.step, EmaModel.update)
    m = build()
    opt = m.configure_optimizers()["optimizer"]
    for step, (r_cond, r_sc) in enumerate([(0.1, 0.2), (0.9, 0.7), (0.1, 0.7)]):
        opt.zero_grad()
        with mg._Inject([noise]), _Draws([t_half], [r_cond, r_sc]):
            loss = m.training_step((h, None, None, u), 0)
        loss.backward()
        torch.nn.utils.clip_grad_norm_(m.model.parameters(), 1.0)
        opt.step()
        m.ema_model.update(m.model)
        out[f"opt::loss{step}"] = loss.detach()
    pn, en = dict(m.model.named_parameters()), dict(m.ema_model.ma_model.named_parameters())
    for n in GRAD_NAMES:
        out[f"opt::param::{n}"] = pn[n].detach()
        out[f"opt::ema::{n}"] = en[n].detach()

    # ---- sample_edm, 50 steps, S_churn 15
    for w in (0.0, 0.5):
        sp = mg.sampler_dict(timesteps=50, S_churn=15.0, w=w)
        m = build(sp)
        m.set_test_sampler_params(mg._wrap(sp))
        hs = fx.randn("cddim/smp/h", B, H, W, 1)
        un = fx.randn("cddim/smp/u_noise", B, H, W, 1)
        steps = [fx.randn(f"cddim/smp/step{i}", B, 1, H, W, dtype="float64") for i in range(50)]
        with torch.no_grad(), mg._Inject(steps):
            xs = m.sample_edm(hs, un, mg._wrap(sp), return_last=False)
        assert xs.dtype == torch.float64 and tuple(xs.shape) == (B, 51, H, W, 1)
        out[f"smp_w{w}::xs_traj"] = xs[:, ::10].contiguous()
    mg.save("cond_ddim.npz", seed=SEED, state_dict_keys=keys, **{k: v for k, v in out.items() if k != "state_dict_keys"})


if __name__ == "__main__":
    main()
