"""Golden vectors for PlCondDdim with PDE guidance (guide_dx=True) in both of its samplers on both networks, made by RUNNING THE
REFERENCE's models/ddim.py PlCondDdim on the CPU with every random draw injected:

  * ``sample``      (:1452-1530, guidance at the current noisy state xt, :1501-1503)  -> xs and x0_preds, fp32
  * ``sample_edm``  (:1532-1601, guidance at the denoised state D, :1576-1578, 1589-1590) -> xs, fp64

on the ADM U-Net (tools/make_golden_cond_ddim.build) and on the DDPM U-Net with the cond_enc head (tools/make_golden_ddpm_cond.build),
B = 3 at 32 x 32, fx.STEP_NORM_STATS, set_pde_loss_function("swe_per", False) (the ``darcy`` case: "darcy"), h_ch = u_ch = 1 (the
reference only sets them inside its step methods).  The cases, sampler blocks, inputs and draws are tests/_cond_guided.py's.

With these random weights the reference's guided runs blow up quickly: the default sigma_max 80 reaches 1e21 after one VP step, ten
DDIM timesteps explode from the sixth step on.  The cases are the tame ones (sigma_max 5 with 6 steps, 5 DDIM timesteps), and before
anything is written the script asserts for each non-Darcy case, with bar = tests/_tol.close_per_entry's (rtol 1e-4, atol 1e-5 x
max|slot|):

  * every compared slot is finite;
  * a rerun with u_noise * (1 + 1e-7) stays within 0.25 x bar on every compared slot (the trajectory is not chaotic at the bar);
  * the guided and the unguided last compared slots differ by >= 100 x bar somewhere (the guidance is visible).

A case that fails the rerun condition on its late slots is compared on its longest qualifying prefix, whose number of steps is
recorded as ``<net>::<tag>::slots`` (xs: slots + 1 entries, x0_preds: slots); a prefix shorter than 4 steps stops the script.  The
Darcy log-probability gradient saturates to exactly 0 on noisy states, so the ``darcy`` case records ``darcy_moved`` (max |guided -
unguided|) and only shows that the route runs; the gradient itself is pinned in tests/test_pde.py.

    python tools/make_golden_cond_guided.py                    # rewrites tests/golden/cond_guided.npz (ADM U-Net) and
                                                               # cond_guided_ddpm.npz (needs the reference checkout)
    python tools/make_golden_cond_guided.py --check adm::ddim  # reruns one case and compares it bit for bit with the stored file
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden_cond_ddim as GA  # noqa: E402  sets up the reference import; the ADM module
import make_golden_ddpm_cond as GD  # noqa: E402  the DDPM module

import numpy as np                  # noqa: E402
import torch                        # noqa: E402

from oracle import fixtures as fx   # noqa: E402
from tests import _cond_guided as G  # noqa: E402

mg = GA.mg
_Uniform = GD._Uniform


def build(net, sp, system):
    st = fx.STEP_NORM_STATS
    if net == "adm":
        m = GA.build(sp)
        m.normalizer_input.set_stats(torch.tensor(st[0]), torch.tensor(st[1]))
        m.normalizer_target.set_stats(torch.tensor(st[2]), torch.tensor(st[3]))
    else:
        m = GD.build(sp, stats=st)
    m.set_pde_loss_function(system, False)
    m.h_ch = m.u_ch = 1
    return m


def run(net, tag, guide, scale=1.0):
    """-> (xs, x0_preds) of ``sample``, (xs, None) of ``sample_edm``; every draw injected."""
    method, system, _ = G.CASES[tag]
    sp = G.sampler_dict(tag, guide_dx=guide)
    m = build(net, sp, system)
    h, un = G.inputs(scale)
    S = G.STEPS[tag]
    if method == "sample":
        with torch.no_grad(), _Uniform([G.eta_draw(tag, k) for k in range(S)]) as inj:
            xs, x0 = m.sample(h, un, mg._wrap(sp), return_last=False, guide_dx=guide)
        assert len(inj.queue) == (0 if abs(sp["eta"]) > 1e-10 else S)
        assert xs.dtype == x0.dtype == torch.float32 and tuple(xs.shape) == (G.B, S + 1, G.H, G.W, 1) and x0.shape[1] == S
        return xs, x0
    m.set_test_sampler_params(mg._wrap(sp))
    with torch.no_grad(), mg._Inject(G.step_draws(tag)) as inj:
        xs = m.sample_edm(h, un, mg._wrap(sp), return_last=False, guide_dx=guide)
    assert not inj.like_queue and xs.dtype == torch.float64 and tuple(xs.shape) == (G.B, S + 1, G.H, G.W, 1)
    return xs, None


def qualifying_steps(got, rerun):
    """The longest prefix (in steps) on which every slot of every compared trajectory is finite and the rerun stays within
    0.25 x bar; and the largest rerun difference in bars on it."""
    S = got[0].shape[1] - 1
    worst, n = 0.0, 0
    for step in range(S + 1):              # xs slot `step`; x0_preds slot step - 1
        slots = [(got[0][:, step], rerun[0][:, step])] + ([(got[1][:, step - 1], rerun[1][:, step - 1])] if got[1] is not None and step else [])
        if not all(bool(torch.isfinite(a).all()) and bool(torch.isfinite(b).all()) for a, b in slots):
            break
        d = max(G.bars_apart(b, a) for a, b in slots)
        if d > 0.25:
            break
        worst, n = max(worst, d), step
    return n, worst


def case(net, tag):
    out = {}
    xs, x0 = run(net, tag, True)
    plain = run(net, tag, False)
    key = f"{net}::{tag}"
    if tag == "darcy":
        assert bool(torch.isfinite(xs).all()) and bool(torch.isfinite(x0).all())
        out[f"{key}::slots"] = np.int64(G.STEPS[tag])
        out[f"{key}::darcy_moved"] = np.float64(float((xs - plain[0]).abs().max()))
        print(f"  {key}: finite, max|x| {float(xs.abs().max()):.3g}, guided - unguided {float(out[f'{key}::darcy_moved']):.3g}")
    else:
        n, worst = qualifying_steps((xs, x0), run(net, tag, True, scale=1.0 + 1e-7))
        assert n >= G.MIN_SLOTS, f"{key}: only {n} steps qualify (finite and rerun within 0.25 x bar); at least {G.MIN_SLOTS} needed"
        moved = G.bars_apart(xs[:, n], plain[0][:, n])
        assert moved >= 100.0, f"{key}: guidance moves slot {n} by {moved:.1f} x bar only"
        out[f"{key}::slots"], out[f"{key}::rerun_bars"], out[f"{key}::moved_bars"] = np.int64(n), np.float64(worst), np.float64(moved)
        print(f"  {key}: {n} of {G.STEPS[tag]} steps compared, max|x| {float(xs[:, :n + 1].abs().max()):.3g}, rerun {worst:.3g} x bar, "
              f"guidance moves slot {n} by {moved:.3g} x bar")
    n = int(out[f"{key}::slots"])
    out[f"{key}::xs"] = xs
    if x0 is not None:
        out[f"{key}::x0_preds"] = x0
    out[f"{key}::unguided_last"] = plain[0][:, n:n + 1].contiguous()
    return out


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--check":
        net, tag = sys.argv[2].split("::")
        stored = np.load(os.path.join(ROOT, "tests", "golden", G.GOLDEN[net]))
        xs, x0 = run(net, tag, True)
        same = np.array_equal(xs.numpy(), stored[f"{net}::{tag}::xs"], equal_nan=True)
        if x0 is not None:
            same = same and np.array_equal(x0.numpy(), stored[f"{net}::{tag}::x0_preds"], equal_nan=True)
        print("bit-identical" if same else "DIFFERENT")
        raise SystemExit(0 if same else 1)
    for net in G.NETS:                     # one file per network: each stays under 1 MB
        out = {}
        for tag in G.cases_of(net):
            out.update(case(net, tag))
        mg.save(G.GOLDEN[net], **out)


if __name__ == "__main__":
    main()
