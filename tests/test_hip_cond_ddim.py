"""GPU: PlCondDdim on the ADM U-Net with self-conditioning (reference models/ddim.py:1053-1605, configs/model/adm_cond_h_res32.yaml)
through the HIP path against the reference's golden vectors (tests/golden/cond_ddim.npz, made by tools/make_golden_cond_ddim.py
with every random draw injected): the self-conditioning forward, the epsilon-prediction training step in its four branches,
three optimiser steps with EMA, the VP-preconditioned Heun sampler."""
import pytest
import torch

from oracle import fixtures as fx
from oracle import mcedm_oracle as orc
from tests._tol import close_per_entry
from tests.test_cond_ddim_cpu import ddim_hparams

pytestmark = pytest.mark.gpu

CFG = orc.UNetConfig(in_channels=1, cond_channels=2, out_ch=1)      # the widened (self-conditioning) parameter table
B, H, W = 3, 32, 32
GRAD_NAMES = ["enc.128x128_conv.weight", "enc.128x128_conv.bias", "out_conv.weight", "dec.32x32_in0.qkv.weight",
              "map_layer0.weight", "map_layer1.bias", "enc.32x32_down.norm0.weight"]
BRANCHES = {"cond_sc": (0.1, 0.2), "cond_nosc": (0.1, 0.7), "nocond_sc": (0.9, 0.2), "nocond_nosc": (0.9, 0.7)}


def make_module(golden, **sampler):
    import mcedm_amd  # noqa: F401
    from mcedm_amd.ddim import PlCondDdim
    hp = ddim_hparams(cond_p=0.8)
    hp.sampler.update(sampler)
    m = PlCondDdim(hp).cuda()
    P = orc.make_params(CFG, int(golden("cond_ddim.npz")["seed"]))
    with torch.no_grad():
        for n, p in m.model.named_parameters():
            p.copy_(P[n])
        for n, p in m.ema_model.ma_model.named_parameters():
            p.copy_(P[n])
    st = fx.TRAIN_NORM_STATS
    m.normalizer_input.set_stats(torch.tensor(st[0]), torch.tensor(st[1]))
    m.normalizer_target.set_stats(torch.tensor(st[2]), torch.tensor(st[3]))
    return m


def train_inputs():
    h = fx.randn("cddim/h", B, H, W, 1) * 0.2 + 1.4
    u = fx.randn("cddim/u", B, H, W, 1) * 0.5
    noise = fx.randn("cddim/noise", B, 1, H, W)
    return h.cuda(), u.cuda(), noise.cuda(), torch.tensor([3, 998])


def run_step(m, monkeypatch, r_cond, r_sc):
    h, u, noise, t_half = train_inputs()
    rands = [r_cond, r_sc]
    with monkeypatch.context() as mp:
        mp.setattr(torch, "randn_like", lambda t, **k: noise.clone())
        mp.setattr(torch, "randint", lambda *a, **k: t_half.clone())
        mp.setattr(torch, "rand", lambda *a, **k: torch.tensor([rands.pop(0)]))
        loss = m.training_step((h, None, None, u), 0)
    assert not rands
    return loss


def close(got, ref, rtol=1e-4, atol=1e-5):
    torch.testing.assert_close(got.detach().cpu(), torch.as_tensor(ref), rtol=rtol, atol=atol)


def test_self_cond_forward_golden(golden):
    """adm_blocks.py:318-338 with labels t in {0, 1, 500, 999} (cosf / sinf of up to 999 rad x freq in the embedding)."""
    g = golden("cond_ddim.npz")
    m = make_module(golden)
    x, cond, xsc = (fx.randn(f"cddim/fwd/{k}", 4, 1, H, W).cuda() for k in ("x", "cond", "xsc"))
    labels = torch.tensor([0.0, 1.0, 500.0, 999.0]).cuda()
    with torch.no_grad():
        for key, c, s in (("fwd_F_sc", cond, xsc), ("fwd_F_nosc", cond, None), ("fwd_F_nocond", None, xsc)):
            F = m.model(x, labels, c, x_self_cond=s)
            close(F, g[key], rtol=1e-4, atol=1e-5 * float(abs(g[key]).max()))


def test_self_cond_forward_is_the_widened_plan_bit_for_bit(golden):
    from mcedm_amd import lib as L
    m = make_module(golden)
    net = m.model
    x, cond, xsc = (fx.randn(f"cddim/fwd/{k}", 4, 1, H, W).cuda() for k in ("x", "cond", "xsc"))
    labels = torch.tensor([0.0, 1.0, 500.0, 999.0]).cuda()
    plan = L.Plan(1, 2, 1, CFG.ch, CFG.ch_mult, CFG.num_res_blocks, CFG.attn_resolutions, CFG.resolution)
    with torch.no_grad():
        packed = plan.pack(net.named_param_dict())
        ref = plan.forward(packed, x, labels, cond=torch.cat([cond, xsc], dim=1).contiguous())
        ref0 = plan.forward(packed, x, labels, cond=torch.cat([cond, torch.zeros_like(xsc)], dim=1).contiguous())
        assert torch.equal(net(x, labels, cond, x_self_cond=xsc), ref)
        assert torch.equal(net(x, labels, cond), ref0)


@pytest.mark.parametrize("tag", list(BRANCHES))
def test_training_step_golden(golden, monkeypatch, tag):
    g = golden("cond_ddim.npz")
    m = make_module(golden)
    loss = run_step(m, monkeypatch, *BRANCHES[tag])
    loss.backward()
    close(loss, g[f"{tag}::loss"], rtol=1e-5, atol=1e-6)
    grads = {n: p.grad for n, p in m.model.named_parameters()}
    for n in GRAD_NAMES:
        ref = torch.as_tensor(g[f"{tag}::grad::{n}"])
        close(grads[n], ref, rtol=1e-3, atol=1e-5 * float(ref.abs().max()))
    sq = torch.tensor([float((gr.double() ** 2).sum()) for gr in grads.values()])
    ref_sq = torch.as_tensor(g[f"{tag}::grad_sqnorm_each"])
    torch.testing.assert_close(sq, ref_sq, rtol=2e-3, atol=1e-10 * float(ref_sq.max()))


def test_training_step_is_bitwise_reproducible(golden, monkeypatch):
    out = []
    for _ in range(2):
        m = make_module(golden)
        loss = run_step(m, monkeypatch, 0.1, 0.2)
        loss.backward()
        out.append((loss.detach().clone(), [p.grad.clone() for p in m.model.parameters()]))
    assert torch.equal(out[0][0], out[1][0])
    assert all(torch.equal(a, b) for a, b in zip(out[0][1], out[1][1]))


def test_three_optimizer_steps_with_ema_golden(golden, monkeypatch):
    from mcedm_amd.optim import FusedAdamEma
    g = golden("cond_ddim.npz")
    m = make_module(golden)
    opt = m.configure_optimizers()["optimizer"]
    assert isinstance(opt, FusedAdamEma)
    for step, (r_cond, r_sc) in enumerate([(0.1, 0.2), (0.9, 0.7), (0.1, 0.7)]):
        def closure():
            opt.zero_grad()
            loss = run_step(m, monkeypatch, r_cond, r_sc)
            loss.backward()
            m.configure_gradient_clipping(opt, 1.0, "norm")
            return loss
        loss = closure()
        m.optimizer_step(0, 0, opt, 0, lambda: loss)
        close(loss, g[f"opt::loss{step}"], rtol=1e-4, atol=1e-6)
    pn, en = dict(m.model.named_parameters()), dict(m.ema_model.ma_model.named_parameters())
    for n in GRAD_NAMES:
        close(pn[n], g[f"opt::param::{n}"], rtol=1e-4, atol=2e-6)
        close(en[n], g[f"opt::ema::{n}"], rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("w", [0.0, 0.5])
def test_sample_edm_golden(golden, monkeypatch, w):
    """PlCondDdim.sample_edm (models/ddim.py:1532-1601): 50 steps, S_churn 15 (every step churns), rounded schedule."""
    g = golden("cond_ddim.npz")
    m = make_module(golden, timesteps=50, S_churn=15.0, w=w)
    sp = m.sparams
    m.set_test_sampler_params(sp)
    hs = fx.randn("cddim/smp/h", B, H, W, 1).cuda()
    un = fx.randn("cddim/smp/u_noise", B, H, W, 1).cuda()
    steps = torch.stack([fx.randn(f"cddim/smp/step{i}", B, 1, H, W, dtype="float64") for i in range(50)]).cuda()
    real = torch.randn
    monkeypatch.setattr(torch, "randn", lambda *a, **k: steps.clone() if k.get("dtype") == torch.float64 else real(*a, **k))
    xs = m.sample_edm(hs, un, sp, return_last=False)
    last = m.sample_edm(hs, un, sp, return_last=True)
    monkeypatch.undo()
    assert xs.dtype == torch.float64 and tuple(xs.shape) == (B, 51, H, W, 1)
    assert torch.equal(last[:, 0], xs[:, -1])
    close_per_entry(xs[:, ::10], g[f"smp_w{w}::xs_traj"], what=f"PlCondDdim.sample_edm w={w}")


def test_vp_sampler_rng_twin_matches_materialised_draws(golden):
    """mcedm_vp_heun_sample_rng == mcedm_vp_heun_sample fed mcedm_normal_fill's draws, bit for bit."""
    from mcedm_amd import lib as L
    m = make_module(golden)
    net = m.ema_model.ma_model
    N = 4
    t = [20.0, 5.0, 1.0, 0.1, 0.0]
    vd = L.vp_sampler_desc(N, 1, t, [25.0, 6.0, 1.0, 0.2], [990.0, 900.0, 800.0, 700.0, 600.0, 500.0, 400.0, 0.0], 1.0, 0.0)
    h = fx.randn("cddim/rng/h", B, 1, H, W).cuda()
    init = fx.randn("cddim/rng/init", B, 1, H, W).cuda()
    seed = torch.tensor([12345], dtype=torch.int64).cuda()
    with torch.no_grad():
        pk = net.packed_weights()
        a = net.plan.vp_sample(pk, vd, h, init, return_last=False, rng_seed=seed)
        steps = torch.stack([L.normal_fill(torch.empty(B, 1, H, W, dtype=torch.float64, device="cuda"), seed, i) for i in range(N)])
        b = net.plan.vp_sample(pk, vd, h, init, steps.contiguous(), return_last=False)
    assert torch.equal(a, b) and torch.isfinite(a).all()


def test_new_entries_run_at_exactly_their_workspace_size(golden, monkeypatch):
    from mcedm_amd import lib as L
    m = make_module(golden, timesteps=4, S_churn=15.0)
    net = m.model
    n_train = net.plan.workspace_bytes(B, H, W, True)
    loss = run_step(m, monkeypatch, 0.1, 0.2)          # the pre-pass and the training forward share one workspace
    assert m._train_ws.buf.numel() == n_train
    loss.backward()
    assert m._train_ws.buf.numel() == n_train
    m.set_test_sampler_params(m.sparams)
    m.sample_edm(fx.randn("cddim/ws/h", B, H, W, 1).cuda(), fx.randn("cddim/ws/u", B, H, W, 1).cuda(), m.sparams)
    assert m._sample_ws.buf.numel() == net.plan.vp_sampler_workspace_bytes(B, H, W)
    assert isinstance(L.REDUCE_SCRATCH_BYTES, int)
