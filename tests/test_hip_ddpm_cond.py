"""GPU: PlCondDdim on the DDPM U-Net ``Model`` with the cond_enc / combine_enc head (configs/model/ddim_cond_h_res32.yaml at 32 x 32)
against the reference's own runs (tests/golden/ddpm_cond*.npz, written by tools/make_golden_ddpm_cond.py with every random draw
injected): the map kernel against the formula in fp64, the forward, get_denoised, both samplers and both evaluation loops, the
device-noise twins, graph replay, batch independence, the folded head against the unfolded one, a checkpoint round trip.
The bar is the project's: rtol 1e-4, atol 1e-5 max|ref| for tensors, tests/_tol.close_per_entry for trajectories."""
import io

import pytest
import torch

from oracle import fixtures as fx
from tests import _ddpm_cond as D
from tests._tol import close_per_entry
from tests.test_hip_eval_steps import _compare
from tests.test_hip_module import wrap

pytestmark = pytest.mark.gpu
B, H, W = D.B, D.H, D.W


def make_module(sampler=None, node_type=False, stats=fx.TRAIN_NORM_STATS):
    import mcedm_amd  # noqa: F401
    from mcedm_amd.ddim import PlCondDdim
    m = PlCondDdim(wrap(D.hparams_dict(sampler, node_type))).cuda()
    return D.fill(m, 2 if node_type else 1, stats)


def close(got, ref, what=""):
    ref = torch.as_tensor(ref)
    torch.testing.assert_close(got.detach().cpu(), ref, rtol=1e-4, atol=1e-5 * float(ref.abs().max()), msg=lambda s: f"{what}: {s}")


@pytest.fixture(scope="module")
def net_module():
    return make_module()


# ---- 1. the map kernel -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cc", [1, 2])
def test_cond_map_against_the_formula_in_fp64(cc):
    """M = (Wc cond_enc.2) (*)circ GELU(cond_enc.0(cond)) + (Wx b_in + Wc b_enc2 + b_comb), everything in fp64 on the host; the
    border ring (where the wrap-around is read), the four corners (both axes wrap) and the interior are held to the bar apart."""
    m = make_module(node_type=cc == 2)
    net = m.model
    cond = D.fwd_inputs(cc)[1]
    with torch.no_grad():
        got = net.plan.cond_map(net.packed_weights(), cond.cuda())
    D.check_cond_map(got, {n: p.detach().cpu().double() for n, p in net.named_parameters()}, cond, f"cc={cc}")


# ---- 2. forward, get_denoised, samplers, evaluation loops against the reference ---------------------------------------------
def test_forward_golden(golden, net_module):
    """Model(x, t, cond, x_self_cond): (cond given / None) x (x_self_cond given / None) at t in {0, 500, 999}, through the module
    and through the C entries (cond_map + forward_cond), which agree bit for bit."""
    g = golden("ddpm_cond.npz")
    net = net_module.model
    x, cond, xsc = (t.cuda() for t in D.fwd_inputs(1))
    with torch.no_grad():
        pk = net.packed_weights()
        cmap = net.plan.cond_map(pk, cond)
        for t in D.T_FWD:
            for ctag, c in (("cond", cond), ("nocond", None)):
                for stag, s in (("sc", xsc), ("nosc", None)):
                    out = net(x, torch.full((B,), t).cuda(), cond=c, x_self_cond=s)
                    close(out, g[f"fwd::{ctag}_{stag}::t{int(t)}"], f"forward {ctag} {stag} t={t}")
                    raw = net.plan.forward_cond(pk, x, t, cond_map=None if c is None else cmap, x_self_cond=s)
                    assert torch.equal(raw, out)


def test_forward_node_type_golden(golden):
    g = golden("ddpm_cond.npz")
    net = make_module(node_type=True).model
    x, cond, xsc = (t.cuda() for t in D.fwd_inputs(2))
    with torch.no_grad():
        close(net(x, torch.full((B,), 500.0).cuda(), cond=cond, x_self_cond=xsc), g["fwd_node::cond_sc::t500"], "node_type forward")


def test_get_denoised_golden(golden, net_module):
    g = golden("ddpm_cond.npz")
    m = net_module
    m.set_test_sampler_params(wrap(D.sampler_dict()))
    _, cond, xsc = (t.cuda() for t in D.fwd_inputs(1))
    xt = fx.randn("ddpmc/den/x", B, 1, H, W).cuda()
    for sg in D.SIGMAS:
        for w in (0.0, 0.5):
            Dx, Fx = m.get_denoised(m.model, xt * sg, torch.tensor(sg, dtype=torch.float64), cond=cond, x_self_cond=xsc, w=w)
            close(Dx, g[f"den::s{sg}::w{w}::D"], f"get_denoised D sigma={sg} w={w}")
            close(Fx, g[f"den::s{sg}::w{w}::F"], f"get_denoised F sigma={sg} w={w}")


def _patch_randn64(monkeypatch, steps):
    real = torch.randn
    monkeypatch.setattr(torch, "randn", lambda *a, **k: steps.clone() if k.get("dtype") == torch.float64 else real(*a, **k))


@pytest.mark.parametrize("w", [0.0, 0.5])
def test_sample_edm_golden(golden, monkeypatch, w):
    """PlCondDdim.sample_edm (models/ddim.py:1532-1601): 18 steps, S_churn 15 (every step churns), every slot of the trajectory."""
    g = golden("ddpm_cond_edm.npz")
    sp = wrap(D.sampler_dict(w=w))
    m = make_module(D.sampler_dict(w=w))
    m.set_test_sampler_params(sp)
    h, un = (t.cuda() for t in D.sample_inputs())
    _patch_randn64(monkeypatch, torch.stack(D.edm_draws("smp", D.EDM_STEPS)).cuda())
    xs = m.sample_edm(h, un, sp, return_last=False)
    last = m.sample_edm(h, un, sp, return_last=True)
    monkeypatch.undo()
    assert xs.dtype == torch.float64 and tuple(xs.shape) == (B, D.EDM_STEPS + 1, H, W, 1)
    assert torch.equal(last[:, 0], xs[:, -1])
    print(f"sample_edm w={w}: worst err / bar {close_per_entry(xs, g[f'w{w}::xs'], what=f'sample_edm w={w}'):.4f}")


@pytest.mark.parametrize("tag", list(D.DDIM_CASES))
def test_sample_golden(golden, monkeypatch, tag):
    """PlCondDdim.sample (:1452-1530): both trajectories, every slot; return_last is the last slot."""
    g = golden("ddpm_cond_ddim.npz")
    N, skip, eta, w = D.DDIM_CASES[tag]
    m = make_module(D.ddim_sampler(N, skip, eta, w))
    h, un = (t.cuda() for t in D.sample_inputs())
    S = D.DDIM_STEPS[tag]
    draws = torch.stack([D.eta_draw(tag, k) for k in range(S)]).cuda()
    real = torch.rand

    def rand(*a, **k):
        shape = tuple(a[0]) if len(a) == 1 and isinstance(a[0], (tuple, list, torch.Size)) else a
        return draws.clone() if shape == tuple(draws.shape) else real(*a, **k)
    monkeypatch.setattr(torch, "rand", rand)
    xs, x0 = m.sample(h, un, m.sparams, return_last=False)
    xs_last, x0_last = m.sample(h, un, m.sparams, return_last=True)
    monkeypatch.undo()
    assert xs.dtype == x0.dtype == torch.float32
    assert tuple(xs.shape) == (B, S + 1, H, W, 1) and tuple(x0.shape) == (B, S, H, W, 1)
    assert torch.equal(xs[:, 0], un)
    print(f"{tag}: xs worst err / bar {close_per_entry(xs, g[f'{tag}::xs'], what=f'{tag} xs'):.4f}, "
          f"x0_preds {close_per_entry(x0, g[f'{tag}::x0_preds'], what=f'{tag} x0_preds'):.4f}")
    assert torch.equal(xs_last[:, 0], xs[:, -1]) and torch.equal(x0_last[:, 0], x0[:, -1])


def _eval_module(sp):
    m = make_module(sp, stats=fx.STEP_NORM_STATS)
    m.set_pde_loss_function("swe_per", False)
    logs = {}
    m.log = lambda name, value, **k: logs.__setitem__(name, torch.as_tensor(value).detach().cpu())
    m.current_epoch = 0
    m.set_test_sampler_params(m.sparams)
    return m, logs


@pytest.mark.parametrize("kind", ["edm", "ddim"])
@pytest.mark.parametrize("step", ["val", "test"])
def test_evaluation_steps_golden(golden, monkeypatch, kind, step):
    """validation_step / test_step (n_samples 2) with ``type: edm`` (18 steps, churn) and ``type: ddim`` (4 steps): every logged
    metric and returned entry."""
    g = golden("ddpm_cond_eval.npz")
    n = D.EVAL_N if step == "test" else 1
    sp = D.sampler_dict() if kind == "edm" else D.ddim_sampler(D.EVAL_DDIM_STEPS)
    m, logs = _eval_module(dict(sp, n_samples=n))
    h, u, init = D.eval_inputs(f"{kind}/{step}", n)
    monkeypatch.setattr(torch, "randn_like", lambda t, **k: init.to(t.device))
    if kind == "edm":
        _patch_randn64(monkeypatch, torch.stack(D.edm_draws(f"{kind}/{step}", D.EDM_STEPS, n * fx.EVAL_B)).cuda())
    batch = (h.cuda(), None, None, u.cuda())
    res = m.validation_step(batch, 0) if step == "val" else m.test_step(batch, 0)
    monkeypatch.undo()
    if step == "val":
        assert res.pop("epoch") == 0
    _compare(g, f"{step}_{kind}", res, logs)


# ---- 3. device-side noise --------------------------------------------------------------------------------------------------
def _vp_desc(w=0.5):
    from mcedm_amd import lib as L
    return L.vp_sampler_desc(4, 1, [20.0, 5.0, 1.0, 0.1, 0.0], [25.0, 6.0, 1.0, 0.2],
                             [990.0, 900.0, 800.0, 700.0, 600.0, 500.0, 400.0, 0.0], 1.0, w)


def _nchw_inputs():
    h, un = D.sample_inputs()
    return h.permute(0, 3, 1, 2).contiguous().cuda(), un.permute(0, 3, 1, 2).contiguous().cuda()


def test_vp_sampler_rng_twin(net_module):
    """mcedm_ddpm_vp_heun_sample_rng == mcedm_ddpm_vp_heun_sample fed mcedm_normal_fill's draws, bit for bit; two seeds differ."""
    from mcedm_amd import lib as L
    net = net_module.ema_model.ma_model
    vd = _vp_desc()
    h, init = _nchw_inputs()
    seed, other = torch.tensor([12345], dtype=torch.int64).cuda(), torch.tensor([12346], dtype=torch.int64).cuda()
    with torch.no_grad():
        pk = net.packed_weights()
        a = net.plan.vp_sample(pk, vd, h, init, return_last=False, rng_seed=seed)
        steps = torch.stack([L.normal_fill(torch.empty(B, 1, H, W, dtype=torch.float64, device="cuda"), seed, i) for i in range(4)])
        b = net.plan.vp_sample(pk, vd, h, init, steps.contiguous(), return_last=False)
        c = net.plan.vp_sample(pk, vd, h, init, return_last=False, rng_seed=other)
    assert torch.equal(a, b) and torch.isfinite(a).all()
    assert torch.equal(a[:, 0], c[:, 0]) and not torch.equal(a[:, -1], c[:, -1])


def _ddim_desc(net_module, eta=0.5, w=0.5, timesteps=4):
    from mcedm_amd import lib as L
    return L.cond_ddim_desc(wrap(D.ddim_sampler(timesteps, eta=eta, w=w)), net_module._alphas_ext(), 1, True)


def test_cond_ddim_rng_twin(net_module):
    """mcedm_ddpm_cond_ddim_sample_rng == mcedm_ddpm_cond_ddim_sample fed mcedm_uniform_fill's draws, bit for bit; two seeds differ."""
    from mcedm_amd import lib as L
    net = net_module.ema_model.ma_model
    dd = _ddim_desc(net_module)
    h, init = _nchw_inputs()
    seed, other = torch.tensor([777], dtype=torch.int64).cuda(), torch.tensor([778], dtype=torch.int64).cuda()
    with torch.no_grad():
        pk = net.packed_weights()
        a = net.plan.cond_ddim_sample(pk, dd, h, init, return_last=False, rng_seed=seed)
        eta = torch.stack([L.uniform_fill(torch.empty(B, 1, H, W, device="cuda"), seed, k) for k in range(4)])
        b = net.plan.cond_ddim_sample(pk, dd, h, init, eta.contiguous(), return_last=False)
        c = net.plan.cond_ddim_sample(pk, dd, h, init, return_last=False, rng_seed=other)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.isfinite(a[0]).all()
    assert not torch.equal(a[0][:, -1], c[0][:, -1])


# ---- 4. graph replay ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["edm", "ddim"])
def test_graph_replay_equals_the_eager_path(monkeypatch, kind):
    """Two calls with different u_noise, replayed from the captured graph (the default; the map is computed inside it) and run
    eagerly (MCEDM_HIP_GRAPH=0): bit for bit, with guidance and noise drawn up front from the same seeds."""
    h, un = (t.cuda() for t in D.sample_inputs())
    noises = [un, fx.randn("ddpmc/smp/u_noise2", B, H, W, 1).cuda()]
    sp = D.sampler_dict(timesteps=4, w=0.5) if kind == "edm" else D.ddim_sampler(4, eta=0.5, w=0.5)
    got = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("MCEDM_HIP_GRAPH", mode)
        m = make_module(sp)
        m.set_test_sampler_params(m.sparams)
        res = []
        for k, nz in enumerate(noises):
            torch.manual_seed(100 + k)
            out = m.sample_edm(h, nz, m.sparams, return_last=False) if kind == "edm" else m.sample(h, nz, m.sparams, return_last=False)[0]
            res.append(out)
        assert (len(m._graphs) == 1 and all(v != "eager" for v in m._graphs.values())) if mode == "1" else not m._graphs
        got[mode] = res
    for a, b in zip(got["1"], got["0"]):
        assert torch.equal(a, b) and torch.isfinite(a).all()
    assert not torch.equal(got["1"][0], got["1"][1])


# ---- 5. batch independence ---------------------------------------------------------------------------------------------------
def test_a_sample_does_not_depend_on_its_batch(net_module):
    """Sample b of the B = 3 call == the B = 1 call on that sample, bit for bit, for both samplers (tensor-fed noise)."""
    net = net_module.ema_model.ma_model
    vd, dd = _vp_desc(), _ddim_desc(net_module)
    h, init = _nchw_inputs()
    steps = torch.stack(D.edm_draws("indep", 4)).cuda()
    eta = torch.stack([D.eta_draw("indep", k) for k in range(4)]).cuda()
    with torch.no_grad():
        pk = net.packed_weights()
        full = net.plan.vp_sample(pk, vd, h, init, steps, return_last=False).clone()
        dfull = [t.clone() for t in net.plan.cond_ddim_sample(pk, dd, h, init, eta, return_last=False)]
        for b in (0, 2):
            one = net.plan.vp_sample(pk, vd, h[b:b + 1].contiguous(), init[b:b + 1].contiguous(), steps[:, b:b + 1].contiguous(),
                                     return_last=False)
            assert torch.equal(one[0], full[b]), b
            xs, x0 = net.plan.cond_ddim_sample(pk, dd, h[b:b + 1].contiguous(), init[b:b + 1].contiguous(),
                                               eta[:, b:b + 1].contiguous(), return_last=False)
            assert torch.equal(xs[0], dfull[0][b]) and torch.equal(x0[0], dfull[1][b]), b


# ---- 6. the fold ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [30.0, 0.05])
def test_folded_head_against_the_unfolded_one(net_module, scale):
    """The same plan evaluated unfolded: x_feat = combine_enc(cat(conv_in(cat(x_self_cond, x)), cond_enc(cond))) composed from the
    module's own torch layers on the device (fp32), handed to the network as its map through a packing whose conv_in weight is
    zero (its folded conv_in is then exactly zero, and with a map the folded bias is not read): everything behind x_feat is
    the same kernels.  Inputs of scale 30 and 0.05."""
    net = net_module.model
    x, cond, xsc = (t.cuda() * scale for t in D.fwd_inputs(1))
    with torch.no_grad():
        feat = net.combine_enc(torch.cat([net.conv_in(torch.cat([xsc, x], 1)), net.cond_enc(cond)], 1)).contiguous()
        params = dict(net.named_parameters())
        params["conv_in.weight"] = torch.zeros_like(params["conv_in.weight"])
        pk0 = net.plan.pack(params, net.timestep_freqs(x.device))
        for t in (0.0, 999.0):
            ref = net.plan.forward_cond(pk0, x, t, cond_map=feat, x_self_cond=xsc)
            got = net(x, torch.full((B,), t).cuda(), cond=cond, x_self_cond=xsc)
            worst = float(D.bars_apart(got.cpu(), ref.cpu()).max())
            print(f"folded vs unfolded, scale {scale}, t {t}: worst err / bar {worst:.4f}")
            close(got, ref.cpu(), f"folded vs unfolded at scale {scale}, t {t}")
        # the map itself: conv_in(0) = b_in, so the unfolded head on a zero input IS M = Wx b_in + Wc cond_enc(cond) + b_comb
        zero_in = net.combine_enc(torch.cat([net.conv_in(torch.zeros_like(torch.cat([xsc, x], 1))), net.cond_enc(cond)], 1))
        close(net.plan.cond_map(net.packed_weights(), cond), zero_in.cpu(), f"map vs the unfolded head at scale {scale}")


# ---- 7. checkpoints ------------------------------------------------------------------------------------------------------------
def test_reference_checkpoint_round_trip(golden, net_module):
    """A state_dict with the reference's keys loads strictly into a fresh module, whose forward then meets the golden."""
    from mcedm_amd.checkpoint import load_reference_checkpoint, save_checkpoint
    g = golden("ddpm_cond.npz")
    assert list(net_module.state_dict().keys()) == [str(k) for k in g["state_dict_keys"]]
    buf = io.BytesIO()
    save_checkpoint(net_module, buf, epoch=3, global_step=7)
    buf.seek(0)
    import mcedm_amd  # noqa: F401
    from mcedm_amd.ddim import PlCondDdim
    fresh = PlCondDdim(wrap(D.hparams_dict())).cuda()
    info = load_reference_checkpoint(fresh, buf, strict=True)
    assert info["epoch"] == 3 and info["global_step"] == 7
    x, cond, xsc = (t.cuda() for t in D.fwd_inputs(1))
    with torch.no_grad():
        out = fresh.ema_model.ma_model(x, torch.full((B,), 500.0).cuda(), cond=cond, x_self_cond=xsc)
        close(out, g["fwd::cond_sc::t500"], "forward after the checkpoint round trip")
        assert torch.equal(out, net_module.model(x, torch.full((B,), 500.0).cuda(), cond=cond, x_self_cond=xsc))
