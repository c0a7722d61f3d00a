"""PlCondDdim with ``hparams.model.dx_cond: True`` (dx_norm 'prob'; reference models/ddim.py:199-204 in ``forward``, :1492 in
``sample``, :1571 / 1584 and get_denoised's :933-934 in ``sample_edm``) on the ADM U-Net with self-conditioning, in both forms of the
dx input (cat_dx True / False), against the reference's own runs (tests/golden/cond_ddim_dx_*.npz, tools/make_golden_cond_ddim_dx.py),
plus the contracts of the new C entries: one step against the same step composed from the op-level entries, the seed form against the
tensor-fed form, graph replay against eager launches, and dx recomputed inside the graph."""
import numpy as np
import pytest
import torch

from oracle import fixtures as fx
from oracle import mcedm_oracle as orc
from tests import _cond_dx as X
from tests import _cond_guided as G
from tests._tol import close_per_entry
from tests.test_cond_ddim_cpu import ddim_hparams
from tests.test_hip_cond_ddim import train_inputs
from tests.test_hip_cond_guided import inject, run
from tests.test_hip_module import wrap

pytestmark = pytest.mark.gpu
B, H, W = X.B, X.H, X.W


def make_module(mode, sp=None, system="swe_per", noise_source="torch", stats=None, dx_cond=True):
    import mcedm_amd  # noqa: F401
    from mcedm_amd.ddim import PlCondDdim
    hp = ddim_hparams(**X.model_update(mode))
    hp.model.dx_cond = dx_cond
    if sp is not None:
        hp.sampler = wrap(dict(sp))
    m = PlCondDdim(hp).cuda()
    P = orc.make_params(X.cfg_of(mode) if dx_cond else X.BASE_CFG, X.SEED)
    assert [n for n, _ in m.model.named_parameters()] == list(P)              # state_dict order of the reference
    with torch.no_grad():
        for mod in (m.model, m.ema_model.ma_model):
            for n, p in mod.named_parameters():
                p.copy_(P[n])
    st = stats or fx.STEP_NORM_STATS
    m.normalizer_input.set_stats(torch.tensor(st[0]).cuda(), torch.tensor(st[1]).cuda())
    m.normalizer_target.set_stats(torch.tensor(st[2]).cuda(), torch.tensor(st[3]).cuda())
    m.set_pde_loss_function(system, False)
    m.noise_source = noise_source
    m.log = lambda *a, **k: None
    return m


def close(got, ref, rtol=1e-4, atol=1e-5):
    torch.testing.assert_close(got.detach().cpu(), torch.as_tensor(ref), rtol=rtol, atol=atol)


# ---- 1. the network ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", X.MODES)
def test_network_forward_golden(golden, mode):
    """adm_blocks.py:319-340: cat(cond, x_self_cond, x, dx), with x_self_cond AND dx and with each of them None (dx None: zeros
    concatenated / zero dx features, not dx_enc(0))."""
    g = golden(X.GOLDEN[mode])
    m = make_module(mode)
    x, cond, xsc, dx, labels = (t.cuda() for t in X.net_inputs())
    with torch.no_grad():
        for key, s, d in (("sc_dx", xsc, dx), ("sc_nodx", xsc, None), ("nosc_dx", None, dx)):
            ref = g[f"{mode}::fwd_F_{key}"]
            close(m.model(x, labels, cond, x_self_cond=s, dx=d), ref, rtol=1e-4, atol=1e-5 * float(abs(ref).max()))
    assert float(abs(g[f"{mode}::fwd_F_sc_dx"] - g[f"{mode}::fwd_F_sc_nodx"]).max()) > 1e-2


# ---- 2. training ---------------------------------------------------------------------------------------------------------
def train_step(m, monkeypatch, branch):
    h, u, noise, t_half = train_inputs()
    rands = list(X.BRANCHES[branch])
    with monkeypatch.context() as mp:
        mp.setattr(torch, "randn_like", lambda t, **k: noise.clone())
        mp.setattr(torch, "randint", lambda *a, **k: t_half.clone())
        mp.setattr(torch, "rand", lambda *a, **k: torch.tensor([rands.pop(0)]))
        loss = m.training_step((h, None, None, u), 0)
    assert not rands                                                         # three draws with dx_cond: dx, cond_p, self-conditioning
    return loss


@pytest.mark.parametrize("branch", list(X.BRANCHES))
@pytest.mark.parametrize("mode", X.MODES)
def test_training_step_golden(golden, monkeypatch, mode, branch):
    """Loss, the stored gradients (dx_enc / combine_enc included) and every parameter's squared gradient norm against the reference's,
    in four branches of the (dx, cond_p, self-conditioning) draws.  dx is evaluated on the noised target, from the cond before the
    cond_p drop, and goes to the pre-pass and to the main pass.

    Measured on one MI355X, worst error in bars (rtol 1e-4, atol 1e-5 x max|ref|) over each case's stored gradients: <= 0.39
    everywhere.  (``map_layer0.weight`` was 0.76 - 1.26 bars in the branches without the pre-pass while the plan's embedding
    frequencies came from the device's powf, 1 ulp off the fp32 power for 7 of 32 of them: 3e-5 in cos / sin(998 * freq).  With the
    frequencies correctly rounded it is 0.06 - 0.39, and the losses agree to the last printed digit.)"""
    g = golden(X.GOLDEN[X.TRAIN_FILE[mode]])
    m = make_module(mode, stats=fx.TRAIN_NORM_STATS)
    loss = train_step(m, monkeypatch, branch)
    loss.backward()
    key = f"{mode}::{branch}"
    print(f"{key}: loss {float(loss):.6f} (reference {float(g[f'{key}::loss']):.6f})")
    close(loss, g[f"{key}::loss"], rtol=1e-4, atol=1e-4)
    grads = {n: p.grad for n, p in m.model.named_parameters()}
    for n in X.grad_names(mode):
        ref = torch.as_tensor(g[f"{key}::grad::{n}"])
        got = X.stored(n, grads[n]).detach().cpu()
        print(f"   {n}: worst err / bar {G.bars_apart(got, ref) if float(ref.abs().max()) > 0 else 0.0:.4f}")
        close(got, ref, rtol=1e-4, atol=1e-5 * max(float(ref.abs().max()), 1e-30))
    sq = torch.tensor([float((gr.double() ** 2).sum()) for gr in grads.values()])
    torch.testing.assert_close(sq, torch.as_tensor(g[f"{key}::grad_sqnorm_each"]).to(sq.dtype), rtol=2e-4, atol=1e-12)
    if mode == "enc" and branch.startswith("nodx"):      # dx None: zero features, no path to dx_enc (adm_blocks.py:355-357)
        assert all(float(grads[n].abs().max()) == 0.0 for n in grads if n.startswith("dx_enc."))
        assert float(grads["combine_enc.weight"].abs().max()) > 0.0


def test_one_optimiser_step_moves_the_dx_encoder(monkeypatch):
    m = make_module("enc", stats=fx.TRAIN_NORM_STATS)
    opt = m.configure_optimizers()["optimizer"]
    before = m.model.dx_enc[0].weight.detach().clone()
    loss = train_step(m, monkeypatch, "dx_cond_sc")
    loss.backward()
    opt.step()
    assert torch.isfinite(m.model.dx_enc[0].weight).all() and not torch.equal(m.model.dx_enc[0].weight.detach(), before)


# ---- 3. the samplers against the reference's trajectories ----------------------------------------------------------------
CASES = [(m, t, False) for m in X.MODES for t in X.SAMPLER_TAGS] + [("enc", t, True) for t in X.GUIDED_TAGS]


@pytest.mark.parametrize("mode,tag,guided", CASES, ids=[X.sampler_key(*c) for c in CASES])
def test_sampler_golden(golden, monkeypatch, mode, tag, guided):
    """Every slot of xs (and of x0_preds for ``sample``) at the trajectory bar (rtol 1e-4, atol 1e-5 x max|slot|); return_last is the
    last slot bit for bit.  Guided cases: the run with the dx description alone (gd NULL) is neither the guided run nor -- like the
    guided run itself -- the reference's run without dx."""
    g = golden(X.GOLDEN["guided" if guided else mode])
    key, S = X.sampler_key(mode, tag, guided), G.STEPS[tag]
    m = make_module(mode, G.sampler_dict(tag), G.CASES[tag][1])
    inject(monkeypatch, tag)
    xs, x0 = run(m, tag, guided)
    xs_last, x0_last = run(m, tag, guided, return_last=True)
    plain = run(m, tag, False)[0] if guided else None
    monkeypatch.undo()
    assert tuple(xs.shape) == (B, S + 1, H, W, 1) and tuple(xs_last.shape) == (B, 1, H, W, 1) and torch.isfinite(xs).all()
    err = close_per_entry(xs, g[f"{key}::xs"], what=f"{key} xs")
    if x0 is not None:
        assert xs.dtype == x0.dtype == torch.float32 and tuple(x0.shape) == (B, S, H, W, 1)
        err = max(err, close_per_entry(x0, g[f"{key}::x0_preds"], what=f"{key} x0_preds"))
        assert torch.equal(x0_last[:, 0], x0[:, -1])
    else:
        assert xs.dtype == torch.float64
    assert torch.equal(xs_last[:, 0], xs[:, -1])
    off = G.bars_apart(xs[:, -1].cpu(), g[f"{key}::nodx_last"][:, 0])
    print(f"{key}: parity worst err / bar {err:.4f}; {off:.4g} x bar away from the reference's run without dx")
    if tag != "darcy":                        # within one bar of a state that the reference holds >= 25 bars away from its dx-off run
        assert off > 20.0
    if guided:
        moved = G.bars_apart(xs[:, -1].cpu(), plain[:, -1].cpu())
        print(f"   guidance on top of dx moves the last slot by {moved:.4g} x bar")
        assert G.bars_apart(plain[:, -1].cpu(), g[f"{key}::nodx_last"][:, 0]) > 1.0
        if tag != "darcy":
            assert moved > 10.0 * max(err, 1.0)


# ---- 4. one step of each entry against the op-level entries ----------------------------------------------------------------
Bs, T1, X1 = 2, 16, 32                        # T != X: the SWE residual runs along W, its time axis along H


def _step_inputs():
    h = fx.randn("cdx/step/h", Bs, T1, X1, 1) * 0.3
    un = fx.randn("cdx/step/u_noise", Bs, T1, X1, 1)
    return h.permute(0, 3, 1, 2).contiguous().cuda(), un.permute(0, 3, 1, 2).contiguous().cuda()


@pytest.mark.parametrize("w", [0.0, 0.5])
@pytest.mark.parametrize("mode", X.MODES)
def test_one_ddim_step_is_its_composition_bit_for_bit(mode, w):
    """mcedm_cond_ddim_sample_dxcond over one timestep = the guidance op on xt -> plan.forward(dx=) (at w = 0.5 a second pass with
    neither cond nor dx) -> mcedm_op_ddim_cond_step.  dx is unscaled, and the first step has dx but no x_self_cond."""
    from mcedm_amd import lib as L
    m = make_module(mode)
    net = m._net(m.ema_model)
    plan, cond, init = net.plan, *_step_inputs()
    ae = torch.tensor([1.0, 0.5, 0.3])
    dd = L.cond_ddim_desc(wrap(dict(timesteps=1, skip_type="uniform", eta=0.0, w=w)), ae, 1, True)
    dxc = m.pde_loss.guidance_desc(m.normalizer_input, m.normalizer_target, T1, X1)
    with torch.no_grad():
        pk = net.packed_weights()
        xs, x0 = plan.cond_ddim_sample(pk, dd, cond, init, return_last=False, dx_input=dxc)
        dx = m.get_dx_input(cond, init)
        labels = torch.zeros(1, device="cuda")
        condp = net.stage_self_cond(cond, None, init)
        F = plan.forward(pk, init, labels, cond=condp, dx=dx)
        Fu = plan.forward(pk, init, labels) if w else None
        a_t = np.float32(0.5)
        s0, s1 = float(np.sqrt(a_t)), float(np.sqrt(np.float32(1.0) - a_t))
        xn = L.op_ddim_cond_step(init, F, s0, s1, 1.0, 0.0, Fu=Fu, w=w)
    assert tuple(dx.shape) == (Bs, 1, T1, X1) and float(dx.abs().max()) > 0.0
    assert tuple(xs.shape) == (Bs, 2, T1, X1, 1) and tuple(x0.shape) == (Bs, 1, T1, X1, 1)
    assert torch.equal(xs[:, 0, ..., 0], init[:, 0])
    assert torch.equal(xs[:, 1, ..., 0], xn[:, 0])
    if w:                                     # the unconditional pass is heard, and it saw neither cond nor dx
        assert not torch.equal(F, Fu)


@pytest.mark.parametrize("w", [0.0, 0.5])
@pytest.mark.parametrize("mode", X.MODES)
def test_one_vp_step_is_its_composition(mode, w):
    """mcedm_vp_heun_sample_dxcond over one step (the last step has no 2nd-order correction) = get_denoised(dx=) on x_hat, whose
    network sees fl(c_in * dx), plus the Euler formula in fp64: x_next = x + (0 - t_hat) * (x - D) / t_hat.  Bound: the three fp64
    operations of the formula, 4 x 2^-53 of the largest operand."""
    from mcedm_amd import lib as L
    sp = G.sampler_dict("vp")
    m = make_module(mode, sp)
    m.set_test_sampler_params(wrap(sp))
    net = m._net(m.ema_model)
    plan, cond, init = net.plan, *_step_inputs()
    sigma = float(m.edm_steps[700])           # a sigma of the schedule table (round_sigma is then the identity)
    vd = L.vp_sampler_desc(1, 1, [sigma, 0.0], [sigma], [m._c_noise(sigma), 0.0], 1.0, w)
    dxc = m.pde_loss.guidance_desc(m.normalizer_input, m.normalizer_target, T1, X1)
    with torch.no_grad():
        xs = plan.vp_sample(net.packed_weights(), vd, cond, init, return_last=False, dx_input=dxc)
        x = init.double() * sigma
        x32 = x.float()
        dx = m.get_dx_input(cond, x32)
        D, _ = m.get_denoised(m.ema_model, x32, torch.tensor(sigma, dtype=torch.float64), cond=cond, dx=dx, w=w)
        D0, _ = m.get_denoised(m.ema_model, x32, torch.tensor(sigma, dtype=torch.float64), cond=cond, dx=None, w=w)
        xn = x + (0.0 - sigma) * ((x - D.double()) / sigma)
    assert xs.dtype == torch.float64 and tuple(xs.shape) == (Bs, 2, T1, X1, 1)
    assert torch.equal(xs[:, 0, ..., 0], x[:, 0])
    err = float((xs[:, 1, ..., 0] - xn[:, 0]).abs().max())
    bound = 4 * 2.0 ** -53 * float(torch.maximum(x.abs(), D.double().abs()).max())
    print(f"vp one step {mode} w={w}: max err {err:.3e}, bound {bound:.3e}; dx moves D by {float((D - D0).abs().max()):.3e}")
    assert err <= bound
    assert float((D - D0).abs().max()) > 1e-3 * float(D.abs().max())


# ---- 5. where the draws come from ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["ddim_cfg_eta", "vp_churn_cfg"])
def test_noise_source_torch_equals_device_fed_the_same_draws(monkeypatch, tag):
    from mcedm_amd import lib as L
    seed, S = 20240611, G.STEPS[tag]
    sampled = G.CASES[tag][0] == "sample"
    dev = make_module("enc", G.sampler_dict(tag), noise_source="device")
    dev._draw_seed = lambda: seed
    a = run(dev, tag, False)
    st = torch.tensor([seed], dtype=torch.int64, device="cuda")
    noise = torch.empty((S, B, 1, H, W), dtype=torch.float32 if sampled else torch.float64, device="cuda")
    for k in range(S):
        (L.uniform_fill if sampled else L.normal_fill)(noise[k], st, k)
    tor = make_module("enc", G.sampler_dict(tag), noise_source="torch")
    real_rand, real_randn = torch.rand, torch.randn
    shape_of = lambda a_: tuple(a_[0]) if len(a_) == 1 and isinstance(a_[0], (tuple, list, torch.Size)) else tuple(a_)      # noqa: E731
    monkeypatch.setattr(torch, "rand", lambda *a_, **k: noise.clone() if sampled and shape_of(a_) == tuple(noise.shape) else real_rand(*a_, **k))
    monkeypatch.setattr(torch, "randn", lambda *a_, **k: noise.clone() if not sampled and shape_of(a_) == tuple(noise.shape) else real_randn(*a_, **k))
    b = run(tor, tag, False)
    monkeypatch.undo()
    for p, q in zip(a, b):
        assert (p is None and q is None) or (torch.equal(p, q) and torch.isfinite(p).all())


# ---- 6. graph replay -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["ddim_cfg_eta", "vp_churn_cfg"])
def test_graph_replay_equals_eager_and_recomputes_dx(monkeypatch, tag):
    """Replay = eager launches bit for bit, a second replay = the first, exactly one graph; and another h between two replays
    changes the result as it changes the eager call's: dx is recomputed inside the graph, not baked in."""
    h2 = fx.randn("cdx/h2", B, H, W, 1) * 0.3
    got = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("MCEDM_HIP_GRAPH", mode)
        m = make_module("enc", G.sampler_dict(tag), noise_source="device")
        m._draw_seed = lambda: 77
        first, again = run(m, tag, True)[0], run(m, tag, True)[0]
        sp = wrap(G.sampler_dict(tag, guide_dx=True))
        un = G.inputs()[1].cuda()
        other = (m.sample(h2.cuda(), un, sp, return_last=False, guide_dx=True)[0] if G.CASES[tag][0] == "sample"
                 else m.sample_edm(h2.cuda(), un, sp, return_last=False, guide_dx=True))
        assert (len(m._graphs) == 1 and all(v != "eager" for v in m._graphs.values())) if mode == "1" else not m._graphs
        assert torch.equal(first, again) and torch.isfinite(first).all()
        got[mode] = (first, other)
    assert torch.equal(got["1"][0], got["0"][0]) and torch.equal(got["1"][1], got["0"][1])
    assert not torch.equal(got["1"][0][:, 1:], got["1"][1][:, 1:])


# ---- 7. a module without dx_cond enqueues what it did -----------------------------------------------------------------------
def test_dx_cond_false_module_has_no_dx_path(golden):
    """The goldens of the module without dx_cond are the existing suites' (tests/test_hip_cond_ddim*.py, test_hip_cond_guided.py); here:
    its calls never reach the dx entries, and its network refuses a dx."""
    from mcedm_amd import lib as L
    m = make_module("enc", G.sampler_dict("ddim"), dx_cond=False)
    assert not m.dx_cond and m._dx_input(G.inputs()[0].cuda()) is None and m.model.plan.dx_mode == L.DX_NONE
    xs, _ = run(m, "ddim", False)
    g = golden(G.GOLDEN["adm"])
    assert torch.isfinite(xs).all() and xs.shape == g["adm::ddim::xs"].shape
    with pytest.raises(NotImplementedError, match="dx_cond=False"):
        m.model(torch.zeros(1, 1, H, W).cuda(), torch.zeros(1).cuda(), dx=torch.zeros(1, 1, H, W).cuda())
