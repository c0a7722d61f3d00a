"""Golden vectors for PlCondDdim on the DDPM U-Net ``Model`` with the cond_enc / combine_enc head (configs/model/ddim_cond_h_res32.yaml
at 32 x 32: ``name: ddim_cond_h``, ``cat_cond: False``, ``cond_channels: 1``, ``self_cond: True``), made by RUNNING THE REFERENCE's
models/ddim.py PlCondDdim on the CPU with every random draw injected.  Four files, each under 1 MB:

  ddpm_cond.npz        state_dict keys (cond_channels 1 and, with node_type, 2); Model(x, t, cond, x_self_cond) for the four
                       (cond given / None) x (x_self_cond given / None) combinations at t in {0, 500, 999}, and the node_type
                       network at t = 500; get_denoised (D, F) at three sigmas with w in {0, 0.5}
  ddpm_cond_edm.npz    sample_edm, 18 steps, S_churn 15 (every step churns), whole trajectories for w in {0, 0.5}
  ddpm_cond_ddim.npz   sample for the four cases of cond_ddim_sample.npz: uniform, quad, uneven, eta 0.5 with w 0.5; xs and x0_preds whole
  ddpm_cond_eval.npz   validation_step and test_step (n_samples 2) with ``type: edm`` and ``type: ddim``: every logged metric and
                       returned entry (keys val_edm::, test_edm::, val_ddim::, test_ddim::)

Parameters and inputs are tagged draws shared with the tests (tests/_ddpm_cond.py).  Before anything is written the script
asserts separation: each swap below moves at least half of the relevant entries by >= 100 x the comparison bar (rtol 1e-4,
atol 1e-5 max|ref|) -- (a) cond zeroed: final state of sample_edm and of sample; (b) cond_enc.2 with zero padding in place of
circular: the border ring of x_feat (and the interior does not move at all); (c) the self-conditioning feedback removed: final
state of sample; (d) w 0 -> 0.5: final state of both samplers.

    python tools/make_golden_ddpm_cond.py      # rewrites tests/golden/ddpm_cond*.npz (needs the reference checkout)
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import make_golden as mg            # noqa: E402  sets up the reference import and the Lightning stand-in

import torch                        # noqa: E402
from models.ddim import PlCondDdim  # noqa: E402  (reference)

from oracle import fixtures as fx   # noqa: E402
from tests import _ddpm_cond as D   # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden_cond_ddim_sample import _Uniform, record  # noqa: E402

B, H, W = D.B, D.H, D.W


def build(sampler=None, node_type=False, stats=fx.TRAIN_NORM_STATS):
    m = PlCondDdim(mg._wrap(D.hparams_dict(sampler, node_type)))
    return D.fill(m, 2 if node_type else 1, stats)


def run_edm(w, zero_cond=False):
    sp = D.sampler_dict(w=w)
    m = build(sp)
    m.set_test_sampler_params(mg._wrap(sp))
    h, un = D.sample_inputs()
    with torch.no_grad(), mg._Inject(D.edm_draws("smp", D.EDM_STEPS)) as inj:
        xs = m.sample_edm(h * 0 if zero_cond else h, un, mg._wrap(sp), return_last=False)
    assert not inj.like_queue and xs.dtype == torch.float64 and tuple(xs.shape) == (B, D.EDM_STEPS + 1, H, W, 1)
    return xs


def run_ddim(tag, timesteps, skip_type, eta, w, zero_cond=False, no_feedback=False):
    sp = D.ddim_sampler(timesteps, skip_type, eta, w)
    m = build(sp)
    h, un = D.sample_inputs()
    if no_feedback:
        net, fwd = m.ema_model.ma_model, m.ema_model.ma_model.forward
        net.forward = lambda x, t, cond=None, x_self_cond=None, dx=None: fwd(x, t, cond=cond, x_self_cond=None, dx=dx)
    with torch.no_grad(), _Uniform([D.eta_draw(tag, k) for k in range(2 * timesteps)]) as inj:
        xs, x0 = m.sample(h * 0 if zero_cond else h, un, mg._wrap(sp), return_last=False)
        used = 2 * timesteps - len(inj.queue)
    assert xs.dtype == x0.dtype == torch.float32 and xs.shape[1] == x0.shape[1] + 1 == D.DDIM_STEPS[tag] + 1 and torch.isfinite(xs).all()
    assert used == (x0.shape[1] if abs(eta) > 1e-10 else 0)
    return xs, x0


def separated(what, other, base):
    share = float((D.bars_apart(other, base) >= 100.0).double().mean())
    print(f"  separation, {what}: {share:.3f} of the entries move by >= 100 x the bar")
    assert share >= 0.5, (what, share)


def x_feat(net, x, cond, xsc):
    return net.combine_cond_feat(net.conv_in(net.cat_conditioning(x, cond, xsc, None)), cond, None)


def golden_net():
    out = {}
    m = build()
    net = m.model
    keys = list(m.state_dict().keys())
    x, cond, xsc = D.fwd_inputs(1)
    with torch.no_grad():
        for t in D.T_FWD:
            tt = torch.full((B,), t)
            for ctag, c in (("cond", cond), ("nocond", None)):
                for stag, s in (("sc", xsc), ("nosc", None)):
                    out[f"fwd::{ctag}_{stag}::t{int(t)}"] = net(x, tt, cond=c, x_self_cond=s)
        # (b) circular padding: the border ring of x_feat moves, the interior does not
        ref = x_feat(net, x, cond, xsc)
        net.cond_enc[2].padding_mode = "zeros"
        net.cond_enc[2]._reversed_padding_repeated_twice = (1, 1, 1, 1)
        zp = x_feat(net, x, cond, xsc)
        ring = torch.ones(H, W, dtype=torch.bool)
        ring[1:-1, 1:-1] = False
        separated("cond_enc.2 zero-padded, border ring of x_feat", zp[..., ring], ref[..., ring])
        assert torch.equal(zp[..., ~ring], ref[..., ~ring])
    m = build()
    m.set_test_sampler_params(mg._wrap(D.sampler_dict()))
    xt = fx.randn("ddpmc/den/x", B, 1, H, W)
    with torch.no_grad():
        for sg in D.SIGMAS:
            for w in (0.0, 0.5):
                Dx, Fx = m.get_denoised(m.model, xt * sg, torch.tensor(sg, dtype=torch.float64), cond=cond, x_self_cond=xsc, w=w)
                out[f"den::s{sg}::w{w}::D"], out[f"den::s{sg}::w{w}::F"] = Dx, Fx
    # node_type: the conditioning is two channels wide
    m2 = build(node_type=True)
    x2, cond2, xsc2 = D.fwd_inputs(2)
    with torch.no_grad():
        out["fwd_node::cond_sc::t500"] = m2.model(x2, torch.full((B,), 500.0), cond=cond2, x_self_cond=xsc2)
    mg.save("ddpm_cond.npz", seed=D.SEED, state_dict_keys=keys, state_dict_keys_node=list(m2.state_dict().keys()), **out)


def golden_edm():
    out = {f"w{w}::xs": run_edm(w) for w in (0.0, 0.5)}
    separated("sample_edm, cond zeroed", run_edm(0.0, zero_cond=True)[:, -1], out["w0.0::xs"][:, -1])
    separated("sample_edm, w 0 -> 0.5", out["w0.5::xs"][:, -1], out["w0.0::xs"][:, -1])
    mg.save("ddpm_cond_edm.npz", seed=D.SEED, **out)


def golden_ddim():
    out = {}
    for tag, (N, skip, eta, w) in D.DDIM_CASES.items():
        out[f"{tag}::xs"], out[f"{tag}::x0_preds"] = run_ddim(tag, N, skip, eta, w)
    base = out["uni::xs"][:, -1]
    N, skip, eta, w = D.DDIM_CASES["uni"]
    separated("sample, cond zeroed", run_ddim("uni", N, skip, eta, w, zero_cond=True)[0][:, -1], base)
    separated("sample, no self-conditioning feedback", run_ddim("uni", N, skip, eta, w, no_feedback=True)[0][:, -1], base)
    separated("sample, w 0 -> 0.5", run_ddim("uni", N, skip, eta, 0.5)[0][:, -1], base)
    mg.save("ddpm_cond_ddim.npz", seed=D.SEED, **out)


def eval_module(sp, logs):
    m = build(sp, stats=fx.STEP_NORM_STATS)
    m.set_pde_loss_function("swe_per", False)
    m.current_epoch = 0
    record(m, logs)
    return m


def golden_eval():
    out = {}
    for kind, sp0 in (("edm", D.sampler_dict()), ("ddim", D.ddim_sampler(D.EVAL_DDIM_STEPS))):
        steps = lambda tag, n: D.edm_draws(tag, D.EDM_STEPS, n * fx.EVAL_B) if kind == "edm" else []      # noqa: E731
        logs = {}
        m = eval_module(sp0, logs)
        m.set_test_sampler_params(mg._wrap(sp0))
        h, u, init = D.eval_inputs(f"{kind}/val", 1)
        with torch.no_grad(), mg._Inject([init] + steps(f"{kind}/val", 1)) as inj:
            res = m.validation_step((h, None, None, u), 0)
        assert not inj.like_queue and res.pop("epoch") == 0
        out.update({f"val_{kind}::{k}": v for k, v in res.items()})
        out.update({f"val_{kind}::log::{k}": v for k, v in logs.items()})

        sp = dict(sp0, n_samples=D.EVAL_N)
        logs = {}
        m = eval_module(sp, logs)
        m.set_test_sampler_params(mg._wrap(sp))
        h, u, init = D.eval_inputs(f"{kind}/test", D.EVAL_N)
        with torch.no_grad(), mg._Inject([init] + steps(f"{kind}/test", D.EVAL_N)) as inj:
            res = m.test_step((h, None, None, u), 0)
        assert not inj.like_queue
        out.update({f"test_{kind}::{k}": v for k, v in res.items()})
        out.update({f"test_{kind}::log::{k}": v for k, v in logs.items()})
    for k, v in out.items():
        if "::log::" in k:
            print(f"  {k} = {float(v):.6g}")
    mg.save("ddpm_cond_eval.npz", seed=D.SEED, **out)


if __name__ == "__main__":
    golden_net()
    golden_edm()
    golden_ddim()
    golden_eval()
