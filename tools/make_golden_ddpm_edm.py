"""Golden vectors for PlCondEdm on the DDPM U-Net ``Model`` with the conditioning concatenated to its input
(configs/model/edm_cond_h_res32.yaml at 32 x 32: ``name: edm_cond_h``, ``cat_cond: True``, ``cond_channels: 1``, ``self_cond: False``),
made by RUNNING THE REFERENCE's models/ddim.py PlCondEdm on the CPU with every random draw injected.  Four files, each under 1 MB:

  ddpm_edm.npz          state_dict keys (cond_channels 1 and, with node_type, 2); Model(x, t, cond) and Model(x, t, None) at three
                        t (one negative, ln 0.05 / 4), and the node_type network; get_denoised (D, F) at three sigmas, w in {0, 0.5}
  ddpm_edm_sample.npz   sample_edm, 18 steps, S_churn 15 (every step churns), whole trajectories for w in {0, 0.5}
  ddpm_edm_guided.npz   sample_edm with guide_dx=True for the SWE residual: the guided trajectory, the unguided final state and the
                        step count (the largest one, at most 18, at which the reference's guided trajectory stays finite)
  ddpm_edm_eval.npz     validation_step and test_step (n_samples 2): every logged metric and returned entry

Parameters and inputs are tagged draws shared with the tests (tests/_ddpm_edm.py).  Before anything is written the script asserts
separation: each swap below moves at least half of the relevant entries by >= 100 x the comparison bar (rtol 1e-4, atol 1e-5
max|ref|) -- (a) cond zeroed: final state of sample_edm; (b) cat(x, cond) in place of cat(cond, x): the network's output; (c) cond
scaled by c_in: F of get_denoised at the three sigmas; (d) VP preconditioning (D = x - sigma F) in place of EDM: D of get_denoised;
(e) w 0 -> 0.5: final state; (f) guide_dx off -> on: final state.

    python tools/make_golden_ddpm_edm.py      # rewrites tests/golden/ddpm_edm*.npz (needs the reference checkout)
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import make_golden as mg            # noqa: E402  sets up the reference import and the Lightning stand-in

import torch                        # noqa: E402
from models.ddim import PlCondEdm   # noqa: E402  (reference)

from oracle import fixtures as fx   # noqa: E402
from tests import _ddpm_edm as D    # noqa: E402

B, H, W = D.B, D.H, D.W


def build(sampler=None, node_type=False, stats=fx.TRAIN_NORM_STATS):
    m = PlCondEdm(mg._wrap(D.hparams_dict(sampler, node_type)))
    m.h_ch, m.u_ch = 1, 1
    return D.fill(m, 2 if node_type else 1, stats)


def separated(what, other, base):
    share = float((D.bars_apart(other, base) >= 100.0).double().mean())
    print(f"  separation, {what}: {share:.3f} of the entries move by >= 100 x the bar")
    assert share >= 0.5, (what, share)


def run_edm(w, zero_cond=False):
    sp = D.sampler_dict(w=w)
    m = build(sp)
    h, un = D.sample_inputs()
    with torch.no_grad(), mg._Inject(D.edm_draws("smp", D.EDM_STEPS)) as inj:
        xs = m.sample_edm(h * 0 if zero_cond else h, un, mg._wrap(sp), return_last=False)
    assert not inj.like_queue and xs.dtype == torch.float64 and tuple(xs.shape) == (B, D.EDM_STEPS + 1, H, W, 1)
    return xs


def golden_net():
    out = {}
    m = build()
    net = m.model
    assert tuple(net.conv_in.weight.shape) == (D.CFG.ch, 2, 3, 3) and net.cond_enc is None and net.combine_enc is None
    keys = list(m.state_dict().keys())
    x, cond = D.fwd_inputs(1)
    with torch.no_grad():
        for k, t in enumerate(D.T_FWD):
            tt = torch.full((B,), t)
            out[f"fwd::cond::t{k}"] = net(x, tt, cond=cond)
            out[f"fwd::nocond::t{k}"] = net(x, tt, cond=None)
        # (b) the order of the concatenation
        base = out["fwd::cond::t1"]
        cat = net.cat_conditioning
        net.cat_conditioning = lambda xx, c, sc, dx: torch.cat((xx, c), dim=1)
        separated("cat(x, cond) in place of cat(cond, x), network output", net(x, torch.full((B,), D.T_FWD[1]), cond=cond), base)
        net.cat_conditioning = cat
    xt = D.den_input()
    Fs, Ds, Fc, Dv = [], [], [], []
    with torch.no_grad():
        for sg in D.SIGMAS:
            sigma = torch.tensor(sg, dtype=torch.float64)
            for w in (0.0, 0.5):
                Dx, Fx = m.get_denoised(m.model, xt * sg, sigma, cond=cond, w=w)
                assert Dx.dtype == Fx.dtype == torch.float32
                out[f"den::s{sg}::w{w}::D"], out[f"den::s{sg}::w{w}::F"] = Dx, Fx
            # (c) cond scaled by c_in, (d) VP preconditioning around the same network evaluation
            s32 = sigma.to(torch.float32).reshape(-1, 1, 1, 1)
            c_in, c_noise = 1 / (1.0 + s32 ** 2).sqrt(), (s32.log() / 4).flatten()
            x32 = (xt * sg).to(torch.float32)
            Fs.append(out[f"den::s{sg}::w0.0::F"]), Ds.append(out[f"den::s{sg}::w0.0::D"])
            Fc.append(m.model(c_in * x32, c_noise, cond=c_in * cond))
            Dv.append(x32 - s32 * Fs[-1])
    separated("cond scaled by c_in, F of get_denoised", torch.stack(Fc), torch.stack(Fs))
    separated("VP preconditioning in place of EDM, D of get_denoised", torch.stack(Dv), torch.stack(Ds))
    # node_type: the conditioning is two channels wide
    m2 = build(node_type=True)
    x2, cond2 = D.fwd_inputs(2)
    with torch.no_grad():
        out["fwd_node::cond::t1"] = m2.model(x2, torch.full((B,), D.T_FWD[1]), cond=cond2)
    mg.save("ddpm_edm.npz", seed=D.SEED, state_dict_keys=keys, state_dict_keys_node=list(m2.state_dict().keys()), **out)


def golden_sample():
    out = {f"w{w}::xs": run_edm(w) for w in (0.0, 0.5)}
    separated("sample_edm, cond zeroed", run_edm(0.0, zero_cond=True)[:, -1], out["w0.0::xs"][:, -1])
    separated("sample_edm, w 0 -> 0.5", out["w0.5::xs"][:, -1], out["w0.0::xs"][:, -1])
    mg.save("ddpm_edm_sample.npz", seed=D.SEED, **out)


def run_guided(N, guide):
    sp = D.sampler_dict(timesteps=N, guide_dx=guide)
    m = build(sp, stats=fx.STEP_NORM_STATS)
    m.set_pde_loss_function(D.GUIDED_SYSTEM, False)
    h, un = D.guided_inputs()
    with torch.no_grad(), mg._Inject(D.edm_draws("gd", N)) as inj:
        xs = m.sample_edm(h, un, mg._wrap(sp), return_last=False, guide_dx=guide)
    assert not inj.like_queue
    return xs


def golden_guided():
    for N in range(D.EDM_STEPS, 1, -1):
        xs = run_guided(N, True)
        if bool(torch.isfinite(xs).all()):
            break
        print(f"  guided {D.GUIDED_SYSTEM}: {N} steps do not stay finite in the reference")
    else:
        raise SystemExit("no step count keeps the guided trajectory finite")
    print(f"  guided {D.GUIDED_SYSTEM}: {N} steps, max|x| {float(xs.abs().max()):.3f}")
    plain = run_guided(N, False)
    separated("sample_edm, guide_dx off -> on", xs[:, -1], plain[:, -1])
    mg.save("ddpm_edm_guided.npz", seed=D.SEED, steps=N, xs=xs, unguided_last=plain[:, -1:].contiguous())


def eval_module(sp, logs):
    m = build(sp, stats=fx.STEP_NORM_STATS)
    m.set_pde_loss_function("swe_per", False)
    m.current_epoch = 0
    m.log = lambda name, value, **k: logs.__setitem__(name, torch.as_tensor(value).detach().clone())
    return m


def golden_eval():
    out = {}
    sp0 = D.sampler_dict()
    logs = {}
    m = eval_module(sp0, logs)
    m.set_test_sampler_params(mg._wrap(sp0))
    h, u, init = D.eval_inputs("val", 1)
    with torch.no_grad(), mg._Inject([init] + D.edm_draws("val", D.EDM_STEPS, fx.EVAL_B)) as inj:
        res = m.validation_step((h, None, None, u), 0)
    assert not inj.like_queue and res.pop("epoch") == 0
    out.update({f"val::{k}": v for k, v in res.items()})
    out.update({f"val::log::{k}": v for k, v in logs.items()})

    sp = dict(sp0, n_samples=D.EVAL_N)
    logs = {}
    m = eval_module(sp, logs)
    m.set_test_sampler_params(mg._wrap(sp))
    h, u, init = D.eval_inputs("test", D.EVAL_N)
    with torch.no_grad(), mg._Inject([init] + D.edm_draws("test", D.EDM_STEPS, D.EVAL_N * fx.EVAL_B)) as inj:
        res = m.test_step((h, None, None, u), 0)
    assert not inj.like_queue
    out.update({f"test::{k}": v for k, v in res.items()})
    out.update({f"test::log::{k}": v for k, v in logs.items()})
    for k, v in out.items():
        if "::log::" in k:
            print(f"  {k} = {float(v):.6g}")
    mg.save("ddpm_edm_eval.npz", seed=D.SEED, **out)


if __name__ == "__main__":
    golden_net()
    golden_sample()
    golden_guided()
    golden_eval()
