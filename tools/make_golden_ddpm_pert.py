"""Golden vectors for the DDPM U-Net ``Model`` (models/ddim_blocks.py:222-470) at ONE TIMESTEP PER SAMPLE, made by RUNNING THE
REFERENCE on the CPU: every row of tests/_ddpm_arch.ALL (B = 2, inputs and parameters of that helper) at t = (3, 937) and at
t = (937, 3), with x_self_cond and cond given wherever the network takes them.

Before anything is written the script asserts, for every row, that the oracle's fp32 forward equals the reference's bit for bit
and that the timesteps matter per sample: swapping the two samples' timesteps moves at least half of the output entries by
>= 100 x the comparison bar (rtol 1e-4, atol 1e-5 max|ref|).  It prints how far the reference's own fp32 output lies from the
fp64 evaluation of the same formula, in units of that bar.  Only the outputs are stored (tests/golden/ddpm_pert.npz).

A second file, tests/golden/ddpm_pert_steps.npz, holds the noising pass of the three modules that sit on this network (PlDdim,
PlCondDdim with the cond_enc head, PlCondEdm with cat_cond; tests/_ddpm_pert.py has the networks, inputs and draws): forward's
(output, x0_t) and training_step's loss for every branch of the draws, every draw injected, each loss also in fp64.

    python tools/make_golden_ddpm_pert.py      # rewrites tests/golden/ddpm_pert*.npz (needs the reference checkout)
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_golden as mg            # noqa: E402  sets up the reference import and the Lightning stand-in

import torch                        # noqa: E402

import make_golden_ddpm_arch as arch  # noqa: E402  build(tag): the reference Model with the row's parameters
from tests import _ddpm_arch as A   # noqa: E402
from tests import _ddpm_pert as T   # noqa: E402


def moved(other, base):
    """share of the entries that lie >= 100 x the bar apart"""
    other, base = other.double(), base.double()
    bar = 1e-5 * float(base.abs().max()) + 1e-4 * base.abs()
    return float(((other - base).abs() / bar >= 100.0).double().mean())


def main():
    torch.set_num_threads(A.CPU_THREADS)
    out = {}
    for tag in A.ALL:
        net, P = arch.build(tag)
        P64 = A.params(tag, torch.float64)
        x, xsc, cond = A.inputs(tag)
        worst = 0.0
        for ts in T.T_PAIRS:
            with torch.no_grad():
                y = net(x, torch.tensor(ts, dtype=torch.float32), cond=cond, x_self_cond=xsc)
            assert y.dtype == torch.float32 and torch.isfinite(y).all()
            assert torch.equal(T.oracle_forward(tag, P, ts), y), f"{T.key(tag, ts)}: the fp32 oracle is not the reference bit for bit"
            worst = max(worst, A.bar_ratio(y, T.oracle_forward(tag, P64, ts)))
            out[T.key(tag, ts)] = y
        share = moved(out[T.key(tag, T.T_PAIRS[1])], out[T.key(tag, T.T_PAIRS[0])])
        assert share >= 0.5, (tag, share)
        print(f"  {tag:14s} max|ref| {float(y.abs().max()):.3f}: timesteps swapped move {share:.3f} of the entries by >= 100 x the bar; "
              f"reference fp32 vs fp64 formula, worst err / bar {worst:.4f}")
    mg.save("ddpm_pert.npz", seed=A.SEED, **out)


class _Draws:
    """torch.rand and torch.randint answered from queues (mg._Inject answers randn_like and randn)"""

    def __init__(self, rands, t_half=None):
        self.rands, self.t_half = list(rands), t_half

    def __enter__(self):
        self._rand, self._randint = torch.rand, torch.randint
        torch.rand = lambda *a, **k: torch.tensor([self.rands.pop(0)])
        torch.randint = lambda *a, **k: self.t_half.clone()
        return self

    def __exit__(self, *a):
        torch.rand, torch.randint = self._rand, self._randint


def golden_steps():
    """forward's (output, x0_t) and training_step's loss of PlDdim, PlCondDdim (cond_enc head) and PlCondEdm (cat_cond) on one small
    DDPM U-Net each, B = 4, for every branch of the draws; next to each loss the same formula in fp64 and the bound a test holds
    the library's loss to: rtol 1e-5 where the reference's own fp32 loss lies within a quarter of that of the fp64 value, else
    4 x the reference's own gap."""
    from models.ddim import PlCondDdim, PlCondEdm, PlDdim      # (reference)
    classes = {"ddim": PlDdim, "cond": PlCondDdim, "edm": PlCondEdm}
    out = {}
    for kind, cls in classes.items():
        h, u = T.step_batch()
        x, cond = T.step_state(kind)
        noise, t_half, rnd = T.step_draws(kind)
        t = T.step_t()
        P64 = T.step_params(kind, torch.float64)
        first = None
        for case, rands in T.STEP_CASES[kind].items():
            m = T.step_fill(cls(mg._wrap(T.step_hparams(kind))), kind)
            m.log = lambda *a, **k: None
            xm = m.data_transform(h, u).permute(0, 3, 1, 2)
            assert torch.equal(xm if kind == "ddim" else xm[:, 1:], x), "the helper's normalisation is not the module's"
            sigma = (rnd * m.P_std + m.P_mean).exp() if kind == "edm" else None
            with torch.no_grad(), _Draws(rands) as d:
                o, x0 = m.forward(x, sigma if kind == "edm" else t, noise, cond=cond)
            assert not d.rands and o.dtype == torch.float32 and tuple(o.shape) == tuple(x.shape)
            with torch.no_grad(), _Draws(rands, t_half) as d, mg._Inject([noise], [rnd]) as inj:
                loss = m.training_step((h, None, None, u), 0)
            assert not d.rands and not inj.like_queue and (kind != "edm" or not inj.randn_queue)
            o64, x64, l64 = T.step_forward64(kind, case, P64)
            gap = abs(float(loss) - float(l64)) / abs(float(l64))
            rtol = 1e-5 if gap <= 0.25e-5 else 4.0 * gap
            print(f"  {kind:5s} {case:12s} loss fp32 {float(loss):.9g}  fp64 {float(l64):.12g}  own gap {gap:.2e} -> rtol {rtol:.2e}; "
                  f"output vs fp64 err / bar {A.bar_ratio(o, o64):.4f}, x0_t {A.bar_ratio(x0, x64):.4f}")
            key = f"{kind}::{case}"
            out.update({f"{key}::output": o, f"{key}::x0_t": x0, f"{key}::loss": loss.reshape(()), f"{key}::loss64": l64.reshape(()),
                        f"{key}::loss_bar": torch.tensor(rtol, dtype=torch.float64)})
            if first is None:           # the timesteps (noise levels) matter per sample: the same forward with them reversed
                first = o
                with torch.no_grad(), _Draws(rands) as d:
                    rev = m.forward(x, sigma.flip(0) if kind == "edm" else t.flip(0), noise, cond=cond)[0]
                share = moved(rev, o)
                print(f"  {kind:5s} levels reversed over the batch move {share:.3f} of the entries by >= 100 x the bar")
                assert share >= 0.5, (kind, share)
    mg.save("ddpm_pert_steps.npz", seed=T.STEP_SEED, **out)


if __name__ == "__main__":
    main()
    golden_steps()
