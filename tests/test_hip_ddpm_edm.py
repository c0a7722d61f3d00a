"""GPU: PlCondEdm on the DDPM U-Net ``Model`` with the conditioning concatenated to its input (configs/model/edm_cond_h_res32.yaml at
32 x 32) against the reference's own runs (tests/golden/ddpm_edm*.npz, written by tools/make_golden_ddpm_edm.py with every random
draw injected): the forward, get_denoised, the sampler with and without PDE guidance, both evaluation loops, the device-noise
twin, graph replay, batch independence, the null conditioning source against a plan without it, a checkpoint round trip.
The bar is the project's: rtol 1e-4, atol 1e-5 max|ref| for tensors, tests/_tol.close_per_entry for trajectories."""
import io

import pytest
import torch

from oracle import fixtures as fx
from tests import _ddpm_edm as D
from tests._tol import close_per_entry
from tests.test_hip_eval_steps import _compare
from tests.test_hip_module import wrap

pytestmark = pytest.mark.gpu
B, H, W = D.B, D.H, D.W


def make_module(sampler=None, node_type=False, stats=fx.TRAIN_NORM_STATS):
    import mcedm_amd  # noqa: F401
    from mcedm_amd.ddim import PlCondEdm
    m = PlCondEdm(wrap(D.hparams_dict(sampler, node_type))).cuda()
    m.noise_source = "torch"
    return D.fill(m, 2 if node_type else 1, stats)


def close(got, ref, what=""):
    ref = torch.as_tensor(ref)
    worst = float(D.bars_apart(got.detach().cpu(), ref).max())
    print(f"{what}: worst err / bar {worst:.4f}")
    torch.testing.assert_close(got.detach().cpu(), ref, rtol=1e-4, atol=1e-5 * float(ref.abs().max()), msg=lambda s: f"{what}: {s}")
    return worst


@pytest.fixture(scope="module")
def net_module():
    return make_module()


# ---- 1. forward, get_denoised, sampler, evaluation loops against the reference ---------------------------------------------
def test_forward_golden(golden, net_module):
    """Model(x, t, cond) and Model(x, t, None) at three t (one negative), through the module and through mcedm_ddpm_forward_cat,
    which agree bit for bit."""
    g = golden("ddpm_edm.npz")
    net = net_module.model
    x, cond = (t.cuda() for t in D.fwd_inputs(1))
    with torch.no_grad():
        pk = net.packed_weights()
        for k, t in enumerate(D.T_FWD):
            tt = torch.full((B,), t).cuda()
            for ctag, c in (("cond", cond), ("nocond", None)):
                out = net(x, tt, cond=c)
                close(out, g[f"fwd::{ctag}::t{k}"], f"forward {ctag} t={t:.4f}")
                assert torch.equal(net.plan.forward_cat(pk, x, float(tt[0]), cond=c), out)


def test_forward_node_type_golden(golden):
    g = golden("ddpm_edm.npz")
    net = make_module(node_type=True).model
    x, cond = (t.cuda() for t in D.fwd_inputs(2))
    with torch.no_grad():
        close(net(x, torch.full((B,), D.T_FWD[1]).cuda(), cond=cond), g["fwd_node::cond::t1"], "node_type forward")


def test_get_denoised_golden(golden, net_module):
    """get_denoised (D, F) at sigma in {0.05, 1.3, 40} for w in {0, 0.5}; model_precond is its D at w = 0."""
    g = golden("ddpm_edm.npz")
    m = net_module
    cond = D.fwd_inputs(1)[1].cuda()
    xt = D.den_input().cuda()
    for sg in D.SIGMAS:
        sigma = torch.tensor(sg, dtype=torch.float64)
        for w in (0.0, 0.5):
            Dx, Fx = m.get_denoised(m.model, xt * sg, sigma, cond=cond, w=w)
            assert Dx.dtype == Fx.dtype == torch.float32
            close(Dx, g[f"den::s{sg}::w{w}::D"], f"get_denoised D sigma={sg} w={w}")
            close(Fx, g[f"den::s{sg}::w{w}::F"], f"get_denoised F sigma={sg} w={w}")
        Dp = m.model_precond(xt * sg, torch.full((B,), sg).cuda(), cond)
        assert torch.equal(Dp, m.get_denoised(m.model, xt * sg, sigma, cond=cond, w=0.0)[0])


def _patch_randn64(monkeypatch, steps):
    real = torch.randn
    monkeypatch.setattr(torch, "randn", lambda *a, **k: steps.clone() if k.get("dtype") == torch.float64 else real(*a, **k))


@pytest.mark.parametrize("w", [0.0, 0.5])
def test_sample_edm_golden(golden, monkeypatch, w):
    """PlCondEdm.sample_edm (models/ddim.py:1532-1601): 18 steps, S_churn 15 (every step churns), every slot of the trajectory."""
    g = golden("ddpm_edm_sample.npz")
    sp = wrap(D.sampler_dict(w=w))
    m = make_module(D.sampler_dict(w=w))
    h, un = (t.cuda() for t in D.sample_inputs())
    _patch_randn64(monkeypatch, torch.stack(D.edm_draws("smp", D.EDM_STEPS)).cuda())
    xs = m.sample_edm(h, un, sp, return_last=False)
    last = m.sample_edm(h, un, sp, return_last=True)
    monkeypatch.undo()
    assert xs.dtype == torch.float64 and tuple(xs.shape) == (B, D.EDM_STEPS + 1, H, W, 1)
    assert torch.equal(last[:, 0], xs[:, -1])
    print(f"sample_edm w={w}: worst err / bar {close_per_entry(xs, g[f'w{w}::xs'], what=f'sample_edm w={w}'):.4f}")


def test_sample_edm_pde_guidance_golden(golden, monkeypatch):
    """guide_dx=True for the SWE residual (models/ddim.py:1576-1578, 1589-1590), at the step count the golden records: the whole
    trajectory; the guided sample differs from the unguided one by more than 10 x the parity error."""
    g = golden("ddpm_edm_guided.npz")
    N = int(g["steps"])
    sp = wrap(D.sampler_dict(timesteps=N, guide_dx=True))
    m = make_module(D.sampler_dict(timesteps=N, guide_dx=True), stats=fx.STEP_NORM_STATS)
    m.set_pde_loss_function(D.GUIDED_SYSTEM, False)
    h, un = (t.cuda() for t in D.guided_inputs())
    _patch_randn64(monkeypatch, torch.stack(D.edm_draws("gd", N)).cuda())
    xs = m.sample_edm(h, un, sp, return_last=False, guide_dx=True)
    plain = m.sample_edm(h, un, sp, return_last=True, guide_dx=False)
    monkeypatch.undo()
    ref = torch.as_tensor(g["xs"])
    print(f"guided sample_edm, {N} steps: worst err / bar {close_per_entry(xs, ref, what='guided sample_edm'):.4f}")
    err = float((xs[:, -1].cpu() - ref[:, -1]).abs().max())
    moved = float((plain[:, 0].cpu() - ref[:, -1]).abs().max())
    print(f"  parity error {err:.3e}, guidance moved the sample by {moved:.3e}")
    close_per_entry(plain, g["unguided_last"], what="unguided sample_edm")
    assert moved > 10 * err, "the guided and unguided samples must differ by far more than the parity error"


@pytest.mark.parametrize("system", ["swe", "darcy"])
def test_sample_edm_guidance_runs_for_the_other_residuals(system):
    """guide_dx=True with the 'swe' and 'darcy' residuals: the call runs, stays finite over its first steps and moves the state."""
    sp = wrap(D.sampler_dict(timesteps=3, S_churn=0.0, guide_dx=True))
    m = make_module(D.sampler_dict(timesteps=3, S_churn=0.0, guide_dx=True), stats=fx.STEP_NORM_STATS)
    m.set_pde_loss_function(system, False)
    h, un = (t.cuda() for t in D.guided_inputs())
    xs = m.sample_edm(h, un, sp, return_last=False, guide_dx=True)
    plain = m.sample_edm(h, un, sp, return_last=False, guide_dx=False)
    assert tuple(xs.shape) == (B, 4, H, W, 1) and torch.isfinite(xs[:, :2]).all()
    assert torch.equal(xs[:, 0], plain[:, 0]) and not torch.equal(xs[:, 1], plain[:, 1])


def _eval_module(sp):
    m = make_module(sp, stats=fx.STEP_NORM_STATS)
    m.set_pde_loss_function("swe_per", False)
    logs = {}
    m.log = lambda name, value, **k: logs.__setitem__(name, torch.as_tensor(value).detach().cpu())
    m.current_epoch = 0
    m.set_test_sampler_params(m.sparams)
    return m, logs


@pytest.mark.parametrize("step", ["val", "test"])
def test_evaluation_steps_golden(golden, monkeypatch, step):
    """validation_step / test_step (n_samples 2), 18 steps with churn: every logged metric and returned entry."""
    g = golden("ddpm_edm_eval.npz")
    n = D.EVAL_N if step == "test" else 1
    m, logs = _eval_module(dict(D.sampler_dict(), n_samples=n))
    h, u, init = D.eval_inputs(step, n)
    monkeypatch.setattr(torch, "randn_like", lambda t, **k: init.to(t.device))
    _patch_randn64(monkeypatch, torch.stack(D.edm_draws(step, D.EDM_STEPS, n * fx.EVAL_B)).cuda())
    batch = (h.cuda(), None, None, u.cuda())
    res = m.validation_step(batch, 0) if step == "val" else m.test_step(batch, 0)
    monkeypatch.undo()
    if step == "val":
        assert res.pop("epoch") == 0
    _compare(g, step, res, logs)


# ---- 2. device-side noise, graph replay, batch independence ------------------------------------------------------------------
def _desc(w=0.5, cond_channels=1):
    """Four steps, two of them churning; c_noise = ln(sigma) / 4 in fp32 at t_hat and at t_next."""
    from mcedm_amd import lib as L
    t, th = [20.0, 5.0, 1.0, 0.1, 0.0], [25.0, 6.0, 1.0, 0.1]
    cn = []
    for i in range(4):
        cn += [float(torch.tensor(th[i]).log() / 4), float(torch.tensor(t[i + 1]).log() / 4) if i < 3 else 0.0]
    return L.vp_sampler_desc(4, cond_channels, t, th, cn, 1.0, w)


def _nchw_inputs():
    h, un = D.sample_inputs()
    return h.permute(0, 3, 1, 2).contiguous().cuda(), un.permute(0, 3, 1, 2).contiguous().cuda()


def test_edm_sampler_rng_twin(net_module):
    """mcedm_ddpm_edm_heun_sample_rng == mcedm_ddpm_edm_heun_sample fed mcedm_normal_fill's draws, bit for bit; two seeds differ."""
    from mcedm_amd import lib as L
    net = net_module.ema_model.ma_model
    vd = _desc()
    h, init = _nchw_inputs()
    seed, other = torch.tensor([12345], dtype=torch.int64).cuda(), torch.tensor([12346], dtype=torch.int64).cuda()
    with torch.no_grad():
        pk = net.packed_weights()
        a = net.plan.edm_sample(pk, vd, h, init, return_last=False, rng_seed=seed)
        steps = torch.stack([L.normal_fill(torch.empty(B, 1, H, W, dtype=torch.float64, device="cuda"), seed, i) for i in range(4)])
        b = net.plan.edm_sample(pk, vd, h, init, steps.contiguous(), return_last=False)
        c = net.plan.edm_sample(pk, vd, h, init, return_last=False, rng_seed=other)
    assert torch.equal(a, b) and torch.isfinite(a).all()
    assert torch.equal(a[:, 0], c[:, 0]) and not torch.equal(a[:, -1], c[:, -1])


@pytest.mark.parametrize("source", ["device", "torch"])
def test_graph_replay_equals_the_eager_path(monkeypatch, source):
    """Two calls with different u_noise, with guidance (w 0.5) and PDE guidance, replayed from the captured graph (the default)
    and run eagerly (MCEDM_HIP_GRAPH=0): bit for bit, the draws keyed or drawn from the same seeds."""
    h, un = (t.cuda() for t in D.guided_inputs())
    noises = [un, fx.randn("ddpme/gd/u_noise2", B, H, W, 1).cuda()]
    sp = D.sampler_dict(timesteps=4, w=0.5, guide_dx=True)
    got = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("MCEDM_HIP_GRAPH", mode)
        m = make_module(sp, stats=fx.STEP_NORM_STATS)
        m.noise_source = source
        m.set_pde_loss_function("swe_per", False)
        res = []
        for k, nz in enumerate(noises):
            torch.manual_seed(100 + k)
            res.append(m.sample_edm(h, nz, m.sparams, return_last=False, guide_dx=True))
        assert (len(m._graphs) == 1 and all(v != "eager" for v in m._graphs.values())) if mode == "1" else not m._graphs
        got[mode] = res
    for a, b in zip(got["1"], got["0"]):
        assert torch.equal(a, b) and torch.isfinite(a).all()
    assert not torch.equal(got["1"][0], got["1"][1])


def test_a_sample_does_not_depend_on_its_batch(net_module):
    """Sample b of the B = 3 call == the B = 1 call on that sample, bit for bit (tensor-fed noise, guidance pass included)."""
    net = net_module.ema_model.ma_model
    vd = _desc()
    h, init = _nchw_inputs()
    steps = torch.stack(D.edm_draws("indep", 4)).cuda()
    with torch.no_grad():
        pk = net.packed_weights()
        full = net.plan.edm_sample(pk, vd, h, init, steps, return_last=False).clone()
        for b in (0, 2):
            one = net.plan.edm_sample(pk, vd, h[b:b + 1].contiguous(), init[b:b + 1].contiguous(), steps[:, b:b + 1].contiguous(),
                                      return_last=False)
            assert torch.equal(one[0], full[b]), b


# ---- 3. a null conditioning source reads as zeros ----------------------------------------------------------------------------
@pytest.mark.parametrize("node_type", [False, True])
def test_null_cond_equals_a_plain_plan_on_the_state_slice(node_type):
    """A cat_cond plan with cond = NULL == the same weights on a plan without conditioning whose conv_in weight is the state
    slice conv_in.weight[:, cond_channels:], bit for bit: forward, denoiser and a sampler call."""
    from mcedm_amd import lib as L
    net = make_module(node_type=node_type).model
    cc = net.cond_channels
    c = D.CFG
    plain = L.DdpmPlan(in_channels=1, out_channels=1, ch=c.ch, ch_mult=c.ch_mult, num_res_blocks=c.num_res_blocks,
                       attn_resolutions=c.attn_resolutions, resolution=c.resolution, self_cond=False)
    params = {n: p.detach() for n, p in net.named_parameters()}
    params["conv_in.weight"] = params["conv_in.weight"][:, cc:].contiguous()
    x = D.fwd_inputs(1)[0].cuda()
    vd = _desc(w=0.5, cond_channels=0)
    init = _nchw_inputs()[1]
    steps = torch.stack(D.edm_draws("null", 4)).cuda()
    with torch.no_grad():
        pk, pk0 = net.packed_weights(), plain.pack(params, net.timestep_freqs(x.device))
        for t in D.T_FWD:
            assert torch.equal(net.plan.forward_cat(pk, x, t), plain.forward(pk0, x, t))
            assert torch.equal(net.plan.forward_cat(pk, x, t), plain.forward_cat(pk0, x, t))
        a = net.plan.edm_denoise(pk, x * 1.3, 1.3, 0.0656, w=0.5, want_F=True)
        b = plain.edm_denoise(pk0, x * 1.3, 1.3, 0.0656, w=0.5, want_F=True)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        assert torch.equal(net.plan.edm_sample(pk, vd, None, init, steps, return_last=False),
                           plain.edm_sample(pk0, vd, None, init, steps, return_last=False))
        # and cond given does move the output: the first source is read
        cond = D.fwd_inputs(cc)[1].cuda()
        assert not torch.equal(net.plan.forward_cat(pk, x, 0.0, cond=cond), net.plan.forward_cat(pk, x, 0.0))


# ---- 4. checkpoints ------------------------------------------------------------------------------------------------------------
def test_reference_checkpoint_round_trip(golden, net_module):
    """A state_dict with the reference's keys loads strictly into a fresh module, whose forward then meets the golden."""
    from mcedm_amd.checkpoint import load_reference_checkpoint, save_checkpoint
    g = golden("ddpm_edm.npz")
    assert list(net_module.state_dict().keys()) == [str(k) for k in g["state_dict_keys"]]
    buf = io.BytesIO()
    save_checkpoint(net_module, buf, epoch=3, global_step=7)
    buf.seek(0)
    import mcedm_amd  # noqa: F401
    from mcedm_amd.ddim import PlCondEdm
    fresh = PlCondEdm(wrap(D.hparams_dict())).cuda()
    info = load_reference_checkpoint(fresh, buf, strict=True)
    assert info["epoch"] == 3 and info["global_step"] == 7
    x, cond = (t.cuda() for t in D.fwd_inputs(1))
    with torch.no_grad():
        tt = torch.full((B,), D.T_FWD[1]).cuda()
        out = fresh.ema_model.ma_model(x, tt, cond=cond)
        close(out, g["fwd::cond::t1"], "forward after the checkpoint round trip")
        assert torch.equal(out, net_module.model(x, tt, cond=cond))
