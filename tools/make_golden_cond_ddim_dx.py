"""Golden vectors for PlCondDdim with ``hparams.model.dx_cond: True`` (dx_norm 'prob') on the ADM U-Net with self-conditioning, in
both forms of the dx input (cat_dx True: 'cat'; False: 'enc', dx_enc / combine_enc), made by RUNNING THE REFERENCE's models/ddim.py
PlCondDdim on the CPU with every random draw injected:

  * DhariwalUNet.forward with x_self_cond AND dx, and with each of them None, labels {0, 1, 500, 999}, B = 4
  * training_step in four branches of the (dx, cond_p, self-conditioning) draws: loss, gradients, every squared gradient norm
  * ``sample`` (:1452-1530, dx_in = get_dx_input(h, xt) at every step, :1492) -> xs and x0_preds, fp32
  * ``sample_edm`` (:1532-1601, dx_in at x_hat and at the Euler x_next, :1571, 1584, scaled by c_in in get_denoised :933) -> xs, fp64
  * the same with guide_dx=True on top (enc), SWE and -- the route only -- Darcy

The parameters are orc.make_params of the widened configuration (the reference's own initialisation has a zero out_conv and shows
nothing); cases, inputs, draws and the bar are tests/_cond_dx.py's and tests/_cond_guided.py's: B = 3 at 32 x 32, 5 DDIM timesteps or 6
VP steps from sigma_max 5.  Before anything is written the script asserts, with bar = tests/_tol.close_per_entry's (rtol 1e-4,
atol 1e-5 x max|slot|):

  * sampler cases: every slot finite; a rerun with u_noise * (1 + 1e-7) within 0.25 x bar on EVERY slot (all steps must qualify: no
    prefix is compared); the run with m.dx_cond = False differs in the last slot by >= 25 x bar.  The ``darcy`` case has neither a
    rerun nor the >= 25 x bar condition: the Darcy log-probability gradient is exactly 0 on noisy states, the case shows that the
    route runs (in enc mode it still differs from dx=None: dx_enc(0) has biases);
  * training: a rerun with noise * (1 + 1e-7) within 0.5 x bar on every stored gradient; the gradients of the dx-on and the dx-off
    branch differ by >= 25 x bar; the queue of injected draws is empty after each step;
  * dx_norm 'l2' raises in the reference (recorded as ``dx_norm_l2_raises``).

    python tools/make_golden_cond_ddim_dx.py                          # rewrites tests/golden/cond_ddim_dx_{cat,enc,guided}.npz
    python tools/make_golden_cond_ddim_dx.py --check enc::vp_churn_cfg   # reruns one sampler case, compares it bit for bit
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden_cond_ddim as GA  # noqa: E402  sets up the reference import
import make_golden_ddpm_cond as GD  # noqa: E402  _Uniform

import numpy as np                  # noqa: E402
import torch                        # noqa: E402
from models.ddim import PlCondDdim  # noqa: E402  (reference)

from oracle import fixtures as fx   # noqa: E402
from oracle import mcedm_oracle as orc  # noqa: E402
from tests import _cond_dx as X     # noqa: E402
from tests import _cond_guided as G  # noqa: E402

mg = GA.mg


def build(mode, sampler=None, system="swe_per", stats=None, dx_norm="prob"):
    hp = GA.hparams(sampler or mg.sampler_dict())
    hp.model.update(X.model_update(mode))
    hp.model.dx_norm = dx_norm
    m = PlCondDdim(hp)
    cfg = X.cfg_of(mode)
    assert [(n, tuple(p.shape)) for n, p in m.model.named_parameters()] == [(n, tuple(s)) for n, s in orc.param_shapes(cfg)]
    P = orc.make_params(cfg, X.SEED)
    with torch.no_grad():
        for mod in (m.model, m.ema_model.ma_model):
            for n, p in mod.named_parameters():
                p.copy_(P[n])
    st = stats or fx.STEP_NORM_STATS
    m.normalizer_input.set_stats(torch.tensor(st[0]), torch.tensor(st[1]))
    m.normalizer_target.set_stats(torch.tensor(st[2]), torch.tensor(st[3]))
    m.set_pde_loss_function(system, False)
    m.h_ch = m.u_ch = 1
    return m


def run(mode, tag, guide=False, scale=1.0, dx_cond=True):
    """-> (xs, x0_preds) of ``sample``, (xs, None) of ``sample_edm``; every draw injected."""
    method, system, _ = G.CASES[tag]
    sp = G.sampler_dict(tag, guide_dx=guide)
    m = build(mode, sp, system)
    m.dx_cond = dx_cond
    h, un = G.inputs(scale)
    S = G.STEPS[tag]
    if method == "sample":
        with torch.no_grad(), GD._Uniform([G.eta_draw(tag, k) for k in range(S)]) as inj:
            xs, x0 = m.sample(h, un, mg._wrap(sp), return_last=False, guide_dx=guide)
        assert len(inj.queue) == (0 if abs(sp["eta"]) > 1e-10 else S)
        assert xs.dtype == x0.dtype == torch.float32 and tuple(xs.shape) == (G.B, S + 1, G.H, G.W, 1) and x0.shape[1] == S
        return xs, x0
    m.set_test_sampler_params(mg._wrap(sp))
    with torch.no_grad(), mg._Inject(G.step_draws(tag)) as inj:
        xs = m.sample_edm(h, un, mg._wrap(sp), return_last=False, guide_dx=guide)
    assert not inj.like_queue and xs.dtype == torch.float64 and tuple(xs.shape) == (G.B, S + 1, G.H, G.W, 1)
    return xs, None


def worst_bars(got, rerun):
    """The largest difference in bars over every slot of every trajectory."""
    worst = 0.0
    for a, b in zip(got, rerun):
        if a is None:
            continue
        assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(b).all())
        worst = max([worst] + [G.bars_apart(b[:, k], a[:, k]) for k in range(a.shape[1])])
    return worst


def sampler_case(mode, tag, guide=False):
    key = X.sampler_key(mode, tag, guide)
    xs, x0 = run(mode, tag, guide)
    assert bool(torch.isfinite(xs).all()) and (x0 is None or bool(torch.isfinite(x0).all())), key
    nodx = run(mode, tag, guide, dx_cond=False)[0]
    out = {f"{key}::xs": xs, f"{key}::nodx_last": nodx[:, -1:].contiguous()}
    if x0 is not None:
        out[f"{key}::x0_preds"] = x0
    moved = G.bars_apart(xs[:, -1], nodx[:, -1])
    if tag == "darcy":
        print(f"  {key}: finite, max|x| {float(xs.abs().max()):.3g}, dx on vs off {moved:.3g} x bar (not a condition)")
    else:
        rerun = worst_bars((xs, x0), run(mode, tag, guide, scale=1.0 + 1e-7))
        assert rerun <= 0.25, f"{key}: the rerun differs by {rerun:.3g} x bar on some slot: not all steps qualify"
        assert moved >= 25.0, f"{key}: dx_cond moves the last slot by {moved:.1f} x bar only"
        out[f"{key}::rerun_bars"] = np.float64(rerun)
        print(f"  {key}: max|x| {float(xs.abs().max()):.3g}, rerun {rerun:.3g} x bar (all steps), dx on vs off {moved:.3g} x bar")
    out[f"{key}::moved_bars"] = np.float64(moved)
    return out


def train_step(mode, branch, scale=1.0):
    h, u, noise, t_half = GA.inputs()
    m = build(mode, stats=fx.TRAIN_NORM_STATS)
    with mg._Inject([noise * scale]) as inj, GA._Draws([t_half], list(X.BRANCHES[branch])) as dr:
        loss = m.training_step((h, None, None, u), 0)
        assert not dr.ints and not dr.rands and not inj.like_queue, (branch, dr.rands)
    loss.backward()
    grads = {n: (torch.zeros_like(p) if p.grad is None else p.grad) for n, p in m.model.named_parameters()}
    return loss.detach(), grads


def training(mode):
    out, kept = {}, {}
    for branch in X.BRANCHES:
        loss, grads = train_step(mode, branch)
        _, again = train_step(mode, branch, scale=1.0 + 1e-7)
        names = X.grad_names(mode)
        live = [n for n in names if float(grads[n].abs().max()) > 0.0]
        rerun = max(G.bars_apart(again[n], grads[n]) for n in live)
        assert rerun <= 0.5, f"{mode}::{branch}: the rerun differs by {rerun:.3g} x bar"
        key = f"{mode}::{branch}"
        out[f"{key}::loss"] = loss
        for n in names:
            out[f"{key}::grad::{n}"] = X.stored(n, grads[n]).contiguous()
        out[f"{key}::grad_sqnorm_each"] = torch.tensor([float((g.double() ** 2).sum()) for g in grads.values()])
        out[f"{key}::rerun_bars"] = np.float64(rerun)
        kept[branch] = grads
        print(f"  {key}: loss {float(loss):.6g}, rerun {rerun:.3g} x bar")
    moved = max(G.bars_apart(kept["dx_cond_sc"][n], kept["nodx_cond_sc"][n]) for n in GA.GRAD_NAMES)
    assert moved >= 25.0, f"{mode}: dx on / off gradients differ by {moved:.1f} x bar only"
    out[f"{mode}::train_moved_bars"] = np.float64(moved)
    print(f"  {mode}: dx-on and dx-off gradients differ by {moved:.3g} x bar")
    return out


def network(mode):
    m = build(mode)
    x, cond, xsc, dx, labels = X.net_inputs()
    with torch.no_grad():
        return {f"{mode}::fwd_F_sc_dx": m.model(x, labels, cond, x_self_cond=xsc, dx=dx),
                f"{mode}::fwd_F_sc_nodx": m.model(x, labels, cond, x_self_cond=xsc),
                f"{mode}::fwd_F_nosc_dx": m.model(x, labels, cond, dx=dx)}


def l2_raises():
    m = build("cat", G.sampler_dict("ddim", guide_dx=False), dx_norm="l2")
    h, un = G.inputs()
    try:
        with torch.no_grad():
            m.sample(h, un, mg._wrap(G.sampler_dict("ddim", guide_dx=False)), return_last=True)
        return 0
    except ValueError as e:
        print("  PlCondDdim.sample with dx_norm='l2' raises in the reference:", str(e)[:90])
        return 1


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--check":
        group, tag = sys.argv[2].split("::")
        mode, guide = ("enc", True) if group == "guided" else (group, False)
        stored = np.load(os.path.join(ROOT, "tests", "golden", X.GOLDEN[group]))
        key = X.sampler_key(mode, tag, guide)
        xs, x0 = run(mode, tag, guide)
        same = np.array_equal(xs.numpy(), stored[f"{key}::xs"])
        if x0 is not None:
            same = same and np.array_equal(x0.numpy(), stored[f"{key}::x0_preds"])
        print("bit-identical" if same else "DIFFERENT")
        raise SystemExit(0 if same else 1)
    files = {g: {} for g in X.GOLDEN}
    assert GA.GRAD_NAMES == X.GRAD_NAMES and GA.SEED == X.SEED and GA.CFG == X.BASE_CFG
    for mode in X.MODES:
        files[mode].update(network(mode))
        for tag in X.SAMPLER_TAGS:
            files[mode].update(sampler_case(mode, tag))
        files[X.TRAIN_FILE[mode]].update(training(mode))
    for tag in X.GUIDED_TAGS:
        files["guided"].update(sampler_case("enc", tag, guide=True))
    files["cat"]["dx_norm_l2_raises"] = torch.tensor(l2_raises())
    assert int(files["cat"]["dx_norm_l2_raises"]) == 1
    for group, out in files.items():
        mg.save(X.GOLDEN[group], seed=X.SEED, **out)
        assert os.path.getsize(os.path.join(ROOT, "tests", "golden", X.GOLDEN[group])) < 1000 * 1000, group


if __name__ == "__main__":
    main()
