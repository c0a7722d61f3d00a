"""Golden vectors for the PDE term of training (PlCondEdm with optimization.pde_loss_lambda > 0, models/ddim.py:1726-1731), made by
RUNNING THE REFERENCE on the CPU with every random draw injected.

  * op level: PlCondEdm.get_pde_loss(h, x0_t, x_gt_unnorm, noise_level, clamp_loss=True, do_rearrange=False) with x0_t a leaf: the
    value and d / d x0_t for every case of tests/_pde_train.py, plus the reference's own fp32 distance from the float64
    restatement (``<case>::ref_err``)
  * module level: training_step on the ADM U-Net (B = 3, 32 x 32): loss, the logged train_loss / train_pde_loss, named gradients
    and per-parameter squared norms; two optimiser steps

The reference's training_step cannot reach the term as it is written: it hands the channel-last h AND the NCHW x0_t to
get_pde_loss with do_rearrange=True (models/ddim.py:1729), whose rearrange (:1396) turns h into (b, w, 1, h), and the
concatenation at :1400 raises.  The tool pins that (``reference_training_step_raises``) and then runs the reference's own
training_step with ONE change: get_pde_loss receives x0_t channel-last and do_rearrange=False, the form the reference's
validation_step / test_step use (:1203, 1297).  Everything else, including the (b, b, t, x) broadcast of pde_loss_prop_t
(:1415-1416), is the reference's code as it stands.

    python tools/make_golden_pde_train.py          # rewrites tests/golden/pde_train.npz (needs the reference checkout)
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import make_golden as mg            # noqa: E402  sets up the reference import and the Lightning stand-in

import torch                        # noqa: E402
from models.ddim import PlCondEdm   # noqa: E402  (reference)

from oracle import fixtures as fx   # noqa: E402
from oracle import mcedm_oracle as orc  # noqa: E402
from tests import _pde_train as T   # noqa: E402

LAMBDA = {"swe_per": 2.0, "darcy": 2.0}            # per system; asserted below to move out_conv.weight's gradient by >= 10 %


def build(system, stats, lam=0.0, use_gt=False, prop_t=False, weights=True):
    hp = mg.make_cond_hparams(fx.CFG_C, mg.sampler_dict())
    hp.optimization.update(pde_loss_lambda=lam, use_gt_pde=use_gt, pde_loss_prop_t=prop_t)
    hp.model.cond_p = T.COND_P
    m = PlCondEdm(hp)
    if weights:
        P = orc.make_params(fx.CFG_C, T.MODULE_SEED)
        with torch.no_grad():
            for n, p in m.model.named_parameters():
                p.copy_(P[n])
            for n, p in m.ema_model.ma_model.named_parameters():
                p.copy_(P[n])
    m.normalizer_input.set_stats(torch.tensor(stats[0]), torch.tensor(stats[1]))
    m.normalizer_target.set_stats(torch.tensor(stats[2]), torch.tensor(stats[3]))
    m.set_pde_loss_function(system, False)
    m.h_ch = m.u_ch = 1
    m.logged = {}
    m.log = lambda k, v, **kw: m.logged.__setitem__(k, v.detach().clone())
    return m


def channel_last_pde_loss(m):
    """The one change (see the module docstring): x0_t goes to get_pde_loss channel-last with do_rearrange=False."""
    orig = m.get_pde_loss
    m.get_pde_loss = lambda cond, x, **kw: orig(cond, x.permute(0, 2, 3, 1), do_rearrange=False, **kw)


def op_level(out):
    bad = []
    mods = {}
    for name, c in T.OP_CASES.items():
        key, st = (c["system"], c["stats"]), c["stats"]
        m = mods[key] = mods[key] if key in mods else build(c["system"], st, weights=False)
        h, D, gt, sigma = T.op_inputs(name)
        x0 = D.permute(0, 2, 3, 1).contiguous().requires_grad_(True)
        val = m.get_pde_loss(h, x0, x_gt_unnorm=gt, noise_level=sigma, clamp_loss=True, do_rearrange=False)
        (g,) = torch.autograd.grad(val, x0)
        g = g.permute(0, 3, 1, 2).contiguous()
        out[f"{name}::value"], out[f"{name}::grad"] = val.detach(), g
        v64, g64 = T.restate(c["system"], h, D, gt, sigma, torch.float64, st)
        ok = torch.isfinite(g) & torch.isfinite(g64)
        out[f"{name}::ref_err"] = torch.tensor(float((g.double() - g64)[ok].abs().max()) if bool(ok.any()) else 0.0)
        # the conditions of a usable case: both sides of the clamp mask, and no cell that fp32 rounding could move across it
        with torch.no_grad():
            x = torch.cat([h * st[1] + st[0], x0 * st[3] + st[2]], dim=-1)
            L = m.pde_loss(x, x if gt is None else gt, m.normalizer_input, m.normalizer_target, clamp_loss=False)
        share = float((L > 1).float().mean())
        near = int(((L - 1).abs() < 1e-3).sum())
        print(f"  {name:32s} value {float(val.detach()):12.5f}  max|grad| {float(g[torch.isfinite(g)].abs().max()) if g.numel() else 0:10.4e}  "
              f"clamped {share:.2f}  |L - 1| < 1e-3: {near}  ref_err {float(out[f'{name}::ref_err']):.2e}")
        if c["degenerate"]:
            assert float(val) == 0.0 and not bool(g.any()), name
        elif not c["dry"] and not c["one_row"]:
            if not (0.1 <= share <= 0.9 and near == 0 and bool(torch.isfinite(g).all())):
                bad.append((name, share, near))
    assert not bad, f"retune tests/_pde_train.py (AMP / RETRY): {bad}"


def train_once(m, system, r_cond):
    h, u, noise, rnd_normal, _ = T.module_inputs(system)
    with mg._Inject([noise], [rnd_normal]), Draws([r_cond]):
        return m.training_step((h, None, None, u), 0)


class Draws:
    """torch.rand replaced by a queue (the cond_p draw of PlCondEdm.forward, models/ddim.py:1683)."""

    def __init__(self, rands):
        self.rands = list(rands)

    def __enter__(self):
        self._r = torch.rand
        torch.rand = lambda *a, **k: torch.tensor([self.rands.pop(0)])
        return self

    def __exit__(self, *a):
        torch.rand = self._r


def module_level(out):
    # the reference as it is: the term cannot be reached
    m = build("swe_per", fx.TRAIN_NORM_STATS, lam=LAMBDA["swe_per"])
    try:
        train_once(m, "swe_per", 0.1)
        raised = 0
    except RuntimeError as e:
        raised = 1
        print(f"  reference training_step with pde_loss_lambda > 0 raises: {str(e)[:110]}")
    assert raised == 1
    out["reference_training_step_raises"] = torch.tensor(raised)

    base = {}
    for tag, (system, use_gt, prop_t, r_cond) in T.MODULE_CASES.items():
        stats = T.module_inputs(system)[4]
        lam = LAMBDA[system]
        m = build(system, stats, lam=lam, use_gt=use_gt, prop_t=prop_t)
        channel_last_pde_loss(m)
        loss = train_once(m, system, r_cond)
        loss.backward()
        grads = {n: p.grad for n, p in m.model.named_parameters()}
        out[f"{tag}::lambda"] = torch.tensor(lam)
        out[f"{tag}::loss"] = loss.detach()
        out[f"{tag}::train_loss"], out[f"{tag}::train_pde_loss"] = m.logged["train_loss"], m.logged["train_pde_loss"]
        for n in T.MODULE_GRAD_NAMES:
            out[f"{tag}::grad::{n}"] = grads[n]
        out[f"{tag}::grad_sqnorm_each"] = torch.tensor([float((g.double() ** 2).sum()) for g in grads.values()])
        # the term must matter: against lambda = 0 it moves out_conv.weight's gradient by at least 10 % in norm
        key = (system, r_cond)
        if key not in base:
            m0 = build(system, stats, lam=0.0)
            l0 = train_once(m0, system, r_cond)
            l0.backward()
            base[key] = dict(m0.model.named_parameters())["out_conv.weight"].grad
        g0 = base[key]
        moved = float((grads["out_conv.weight"] - g0).norm() / g0.norm())
        print(f"  {tag:12s} loss {float(loss):.6f} = edm {float(m.logged['train_loss']):.6f} + {lam:g} * pde "
              f"{float(m.logged['train_pde_loss']):.4f}; out_conv.weight gradient moved by {moved:.3f}")
        assert moved >= 0.1, (tag, moved)

    # two optimiser steps (Lightning: closure, clip_grad_norm_(1.0), Adam.step, EmaModel.update)
    system = "swe_per"
    m = build(system, fx.TRAIN_NORM_STATS, lam=LAMBDA[system])
    channel_last_pde_loss(m)
    opt = m.configure_optimizers()["optimizer"]
    for step, r_cond in enumerate(T.OPT_DRAWS):
        opt.zero_grad()
        loss = train_once(m, system, r_cond)
        loss.backward()
        torch.nn.utils.clip_grad_norm_(m.model.parameters(), 1.0)
        opt.step()
        m.ema_model.update(m.model)
        out[f"opt::loss{step}"] = loss.detach()
    pn, en = dict(m.model.named_parameters()), dict(m.ema_model.ma_model.named_parameters())
    for n in T.MODULE_GRAD_NAMES:
        out[f"opt::param::{n}"] = pn[n].detach()
        out[f"opt::ema::{n}"] = en[n].detach()


def main():
    out = {}
    op_level(out)
    module_level(out)
    mg.save("pde_train.npz", seed=T.MODULE_SEED, **out)


if __name__ == "__main__":
    main()
