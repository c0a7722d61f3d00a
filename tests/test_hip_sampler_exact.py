"""GPU: every sampler entry's step arithmetic against the reference's own, bit for bit, on a network that returns a constant.

With every parameter zero except the bias of the last convolution both U-Nets return that bias (tests/test_sampler_exact_cpu.py
shows it for the oracle's networks; test_device_networks_return_the_bias for the device's), so a sampler is a closed-form
recurrence in fp32 / fp64 and the oracle's loops compute it on the CPU without a network noise floor.  Every case compares the
whole returned tensor with torch.equal -- with return_last == 0 and once more with return_last == 1 -- and prints the largest
difference in ulps of the output dtype first.  The schedules come from the library's host helpers, are held to 2 ulp of the
oracle's and are fed to the reference loop, so that a host pow's last place does not leak into the comparison.  The reference
loops run under _sampler_exact.ieee_sqrt: torch's CPU square root is not correctly rounded and differs between hosts, the
kernels' and the library's is (without it 13 of 25 cases differed on the test host, each by the last place of an fp32 root; with it none does).
The churn draws are materialised tensors (the _rng forms are tied to these bit for bit in tests/test_hip_sampler_noise.py and
test_hip_device_noise.py).

What this covers: the fp64 state updates, the churn window (S_min, S_max), S_noise, the index of the step_noise slice when only
some steps churn, rho and sigma_data, fractional masks, the Euler-only last step and timesteps == 1, classifier-free blending and
the preconditioning around F, the fp32 PDE-guidance term, the RePaint re-noising with both fields partly known, the DDIM step and
its noise coefficients, the 'b t h w c' trajectory stores with C == 1, H != W and past the 2048 x 256 threads of the grid cap.

What it does NOT cover: a constant network hides everything the network READS -- c_in, c_noise, the routing of cond, the second
(unconditional) pass of classifier-free guidance, the self-conditioning feedback.  Those stay with the golden tests
(test_hip_e2e.py, test_hip_cond_edm.py, test_hip_cond_ddim*.py, test_hip_cond_guided.py, test_hip_ddpm*.py)."""
import types

import numpy as np
import pytest
import torch

from oracle import ddpm_oracle as ddo
from oracle import fixtures as fx
from oracle import mcedm_oracle as orc
from tests import _sampler_exact as E

pytestmark = pytest.mark.gpu
B, H, W, R = E.B, E.H, E.W, E.R


# ---- one plan and one pack (plus its zero-bias twin) per network ----------------------------------------------------------
def _adm(cfg):
    import mcedm_amd  # noqa: F401
    from mcedm_amd import lib as L
    assert torch.cuda.is_available()
    plan = L.Plan(cfg.in_channels, cfg.cond_channels, cfg.out_ch, cfg.ch, cfg.ch_mult, cfg.num_res_blocks, cfg.attn_resolutions,
                  cfg.resolution)
    P = E.constant_params(orc.make_params, cfg, E.bias_of(cfg))
    P0 = E.constant_params(orc.make_params, cfg, E.bias_of(cfg, zero=True))
    return types.SimpleNamespace(L=L, plan=plan, cfg=cfg, P=P, P0=P0, packed=plan.pack({k: v.cuda() for k, v in P.items()}),
                                 packed0=plan.pack({k: v.cuda() for k, v in P0.items()}))


def _ddpm(cfg):
    import mcedm_amd  # noqa: F401
    from mcedm_amd import lib as L
    assert torch.cuda.is_available()
    plan = L.DdpmPlan(cfg.in_channels, cfg.out_ch, cfg.ch, cfg.ch_mult, cfg.num_res_blocks, cfg.attn_resolutions, cfg.resolution,
                      self_cond=cfg.self_cond, cond_channels=cfg.cond_channels, cat_cond=cfg.cat_cond)
    P = E.constant_params(ddo.make_params, cfg, E.bias_of(cfg))
    assert plan.param_names == [n for n, _ in ddo.param_shapes(cfg)]
    packed = plan.pack({k: v.cuda() for k, v in P.items()}, ddo.timestep_freqs(cfg.ch).cuda())
    return types.SimpleNamespace(L=L, plan=plan, cfg=cfg, P=P, packed=packed)


@pytest.fixture(scope="module")
def joint():
    return _adm(E.CFG_JOINT)


@pytest.fixture(scope="module")
def single():
    return _adm(E.CFG_SINGLE)


@pytest.fixture(scope="module")
def wide():
    return _adm(E.CFG_WIDE)


@pytest.fixture(scope="module")
def d_joint():
    return _ddpm(E.CFG_D_JOINT)


@pytest.fixture(scope="module")
def d_head():
    return _ddpm(E.CFG_D_HEAD)


@pytest.fixture(scope="module")
def d_cat():
    return _ddpm(E.CFG_D_CAT)


def _both(call, ref_of, what):
    """The whole trajectory and the return_last form of one sampler call against the reference's: -> the trajectory (CPU)."""
    with torch.no_grad():
        for last in (False, True):
            got = call(last)
            with E.ieee_sqrt():
                ref = ref_of(last)
            if isinstance(got, tuple):
                for name, g, r in zip(("xs", "x0_preds"), got, ref):
                    E.check_exact(f"{what} {name} return_last={int(last)}", g, r)
            else:
                E.check_exact(f"{what} return_last={int(last)}", got, ref)
            if not last:
                full = got
    return tuple(t.cpu() for t in full) if isinstance(full, tuple) else full.cpu()


def _guidance(L):
    """SweFvLoss on identity normalisers (x_unnorm = x * 1 + 0 is exact), 8 rows of 12 cells: the C description and the same
    gradient through the library's own mcedm_swe_fv_guidance as the reference loop's callable (h, D[f64]) -> dx [B, 1, H, W]."""
    half_dt, dx = float(np.float32(0.001)), float(np.float32(1.0 / W))
    gd = L.GuidanceDesc(1, half_dt, dx, 0.0, 0.0, 1.0, 0.0, 1.0, 5.0)

    def guide(h, D):
        x_un = torch.cat([h[:, :1].float().permute(0, 2, 3, 1), D.float().permute(0, 2, 3, 1)], dim=-1).contiguous().cuda()
        g = L.swe_fv_guidance(x_un, x_un, half_dt, dx, 1.0, 1.0).cpu()
        return torch.mean(g.permute(0, 3, 1, 2), dim=1, keepdim=True)      # get_dx_pde's mean over the two field gradients
    return gd, guide


def _water(tag, *shape):
    """A positive conditioning field (the SWE residual takes its square root)."""
    return 1.5 + 0.25 * fx.randn(f"exact/{tag}/h", *shape).clamp(-1.9, 1.9)


# ---- 0. the premise, on the device ----------------------------------------------------------------------------------------
def test_device_networks_return_the_bias(joint, single, wide, d_joint, d_head, d_cat):
    for n in (joint, single, wide):
        c = n.cfg
        x = (fx.randn("exact/premise/x", B, c.in_channels, H, W) * 80.0).cuda()
        cond = fx.randn("exact/premise/cond", B, c.cond_channels, H, W).cuda()
        want = torch.tensor(E.bias_of(c)).view(1, -1, 1, 1).expand(B, -1, H, W)
        for cc in (cond, None):
            assert torch.equal(n.plan.forward(n.packed, x, torch.tensor([0.3, -1.2, 1.1]).cuda(), cond=cc).cpu(), want)
        assert torch.equal(n.plan.forward(n.packed0, x, torch.tensor([0.3]).cuda(), cond=cond).cpu(), torch.zeros_like(want))
    for n in (d_joint, d_head, d_cat):
        c = n.cfg
        x = (fx.randn("exact/premise/dx", B, c.in_channels, R, R) * 80.0).cuda()
        cond = fx.randn("exact/premise/dcond", B, 1, R, R).cuda()
        want = torch.tensor(E.bias_of(c)).view(1, -1, 1, 1).expand(B, -1, R, R)
        if c.cat_cond:
            outs = [n.plan.forward_cat(n.packed, x, 937.0, cond=cond), n.plan.forward_cat(n.packed, x, 3.0)]
        elif c.cond_channels:
            outs = [n.plan.forward_cond(n.packed, x, 937.0, cond_map=n.plan.cond_map(n.packed, cond), x_self_cond=x),
                    n.plan.forward_cond(n.packed, x, 3.0)]
        else:
            outs = [n.plan.forward(n.packed, x, 937.0, x_self_cond=x), n.plan.forward(n.packed, x, 3.0)]
        for o in outs:
            assert torch.equal(o.cpu(), want)


# ---- 1. mcedm_heun_sample ----------------------------------------------------------------------------------------------------
def _window_desc(L, w, S_churn=None, timesteps=None):
    kw = dict(E.WINDOW, w=w)
    if S_churn is not None:
        kw["S_churn"] = S_churn
    if timesteps is not None:
        kw["timesteps"] = timesteps
    sp = orc.SamplerParams(**kw)
    sd = L.sampler_desc(sp, sigma_data=E.SIGMA_DATA)
    t = L.edm_t_steps(sd)
    assert E.within_ulps(t, orc.edm_t_steps(sp.timesteps, sp.sigma_min, sp.sigma_max, sp.rho).tolist()), t
    return sp, sd, t


@pytest.mark.parametrize("churn", [True, False], ids=["churn", "plain"])
@pytest.mark.parametrize("w", [0.0, 0.5, E.W_ODD])
def test_heun_masked(joint, w, churn):
    """PlMcedm.sample_edm with a 0 / 0.75 / 1 mask, the churn window in the middle of the schedule, S_noise 1.007, rho 5,
    sigma_data 0.5; plain: S_churn 0 with step_noise NULL.  w = 0.32: the blend's factor is fl32(w + 1), the sum formed in
    double (the finishing kernel once added 1 to fl32(w): the neighbouring fp32 number for this w)."""
    L, n = joint.L, joint
    sp, sd, t = _window_desc(L, w, S_churn=None if churn else 0.0)
    assert E.churns(t, sp.S_churn, sp.S_min, sp.S_max) == (E.WINDOW_CHURNS if churn else [False] * 6)
    shape = (B, 2, H, W)
    cond, init = fx.randn("exact/masked/cond", *shape), fx.randn("exact/masked/init", *shape)
    mask = E.fractional_mask("masked", shape)
    assert all(bool((mask[:, c] == v).any()) for c in range(2) for v in (0.0, 0.75, 1.0))
    steps = E.draws64("masked", sp.timesteps, shape) if churn else None
    dev_steps = torch.stack(steps).cuda() if churn else None
    xs = _both(lambda last: n.plan.sample(n.packed, sd, cond.cuda(), mask.cuda(), init.cuda(), dev_steps, return_last=last),
               lambda last: orc.sample_edm(n.P, n.cfg, cond, mask, sp, init, steps, return_last=last, sigma_data=E.SIGMA_DATA, t_steps=t),
               f"heun_sample masked w={w} {'churn' if churn else 'plain'}")
    known = (mask == 0).permute(0, 2, 3, 1)
    for slot in range(xs.shape[1]):            # where the mask is 0 the state IS the conditioning, in every slot
        assert torch.equal(xs[:, slot][known], cond.permute(0, 2, 3, 1).double()[known])


@pytest.mark.parametrize("case", ["window", "two_steps"])
def test_heun_unmasked(single, case):
    """PlCondEdm.sample_edm (mask NULL, C = 1) on the window schedule with w = 0.5, and on the shortest schedule the entry takes
    (two steps: one Heun step and the Euler-only last one)."""
    L, n = single.L, single
    sp, sd, t = _window_desc(L, 0.5, timesteps=None if case == "window" else 2)
    shape = (B, 1, H, W)
    h, init = fx.randn("exact/unmasked/h", *shape), fx.randn("exact/unmasked/init", *shape)
    steps = E.draws64("unmasked", sp.timesteps, shape)
    assert any(E.churns(t, sp.S_churn, sp.S_min, sp.S_max)) == (case == "window")
    dev_steps = torch.stack(steps).cuda()
    _both(lambda last: n.plan.sample(n.packed, sd, h.cuda(), None, init.cuda(), dev_steps, return_last=last),
          lambda last: orc.sample_edm_cond(n.P, n.cfg, h, sp, init, steps, return_last=last, sigma_data=E.SIGMA_DATA, t_steps=t),
          f"heun_sample unmasked {case}")


def test_heun_rejects_one_timestep(single):
    """timesteps == 1 divides 0 by 0 in the schedule expression (mcedm.py:584, ddim.py:1551: idx / (num_steps - 1)): the entry
    and its schedule helper refuse it instead of sampling on NaN.  The Euler-only single step itself is exercised where the
    schedule is the caller's: test_vp_heun[one_step], test_ddpm_edm_heun[one_step]."""
    L, n = single.L, single
    sd = L.sampler_desc(orc.SamplerParams(timesteps=1), sigma_data=E.SIGMA_DATA)
    with pytest.raises(RuntimeError, match="timesteps=1"):
        L.edm_t_steps(sd)
    with pytest.raises(RuntimeError, match="timesteps=1"):
        n.plan.sample(n.packed, sd, torch.zeros(B, 1, H, W).cuda(), None, torch.zeros(B, 1, H, W).cuda(), None)


def test_heun_guided_swe(single):
    """mcedm_heun_sample_guided: d -= fl(fl(weight * dx) / fl32(t_hat)) in fp32, both stages dividing by t_hat."""
    L, n = single.L, single
    gd, guide = _guidance(L)
    sp, sd, t = _window_desc(L, 0.0)
    shape = (B, 1, H, W)
    h, init = _water("guided", *shape), fx.randn("exact/guided/init", *shape)
    steps = E.draws64("guided", sp.timesteps, shape)
    dev_steps = torch.stack(steps).cuda()
    xs = _both(lambda last: n.plan.sample(n.packed, sd, h.cuda(), None, init.cuda(), dev_steps, return_last=last, guidance=gd),
               lambda last: orc.sample_edm_cond(n.P, n.cfg, h, sp, init, steps, return_last=last, guidance=guide,
                                                sigma_data=E.SIGMA_DATA, t_steps=t),
               "heun_sample_guided swe")
    with torch.no_grad(), E.ieee_sqrt():
        plain = orc.sample_edm_cond(n.P, n.cfg, h, sp, init, steps, return_last=False, sigma_data=E.SIGMA_DATA, t_steps=t)
    assert torch.isfinite(xs).all() and not torch.equal(xs[:, 1], plain[:, 1])      # the guidance term is there


def test_heun_past_the_grid_cap(joint):
    """5 x 2 x 232 x 228 = 528,960 state elements against the 2048 x 256 = 524,288 threads every state kernel is capped at: the
    grid-stride loops take a second trip, the stores of three trajectory slots reach 12.7 MB.  The reference loop runs with the
    constant F substituted for the oracle network (tests/test_sampler_exact_cpu.py: the network returns it exactly)."""
    L, n = joint.L, joint
    Bb, Hb, Wb = E.BIG
    assert Bb * 2 * Hb * Wb > 2048 * 256
    sp = orc.SamplerParams(timesteps=2, S_churn=15.0, S_noise=1.007, w=0.0)
    sd = L.sampler_desc(sp, sigma_data=E.SIGMA_DATA)
    t = L.edm_t_steps(sd)
    assert E.within_ulps(t, orc.edm_t_steps(2, sp.sigma_min, sp.sigma_max, sp.rho).tolist())
    shape = (Bb, 2, Hb, Wb)
    cond, init = fx.randn("exact/big/cond", *shape), fx.randn("exact/big/init", *shape)
    mask = E.fractional_mask("big", shape)
    steps = E.draws64("big", 2, shape)
    got = n.plan.sample(n.packed, sd, cond.cuda(), mask.cuda(), init.cuda(), torch.stack(steps).cuda(), return_last=False)
    with torch.no_grad(), E.ieee_sqrt():
        ref = orc.sample_edm(None, n.cfg, cond, mask, sp, init, steps, return_last=False, sigma_data=E.SIGMA_DATA, t_steps=t,
                             net=E.const_net(E.bias_of(n.cfg)))
    E.check_exact("heun_sample 5 x 232 x 228", got, ref)


# ---- 2. mcedm_vp_heun_sample[_guided] ------------------------------------------------------------------------------------------
VP_CASES = {"w0": (E.VP_SIGMAS, 0.0, False), "cfg": (E.VP_SIGMAS, 0.5, False), "w_odd": (E.VP_SIGMAS, E.W_ODD, False),
            "bias0": (E.VP_SIGMAS, 0.5, True), "one_step": (E.ONE_STEP, 0.5, False)}


@pytest.mark.parametrize("case", list(VP_CASES))
def test_vp_heun(wide, case):
    """PlCondDdim.sample_edm: one step churns and one does not, S_noise 0.9; bias0: D == x32 exactly, so the slope is the
    rounding residue of the fp64 state alone; one_step: timesteps == 1, Euler only."""
    L, n = wide.L, wide
    (sig, hat), w, zero = VP_CASES[case]
    t, th, c = E.vp_schedule(E.ddpm_tables()[0], sig, hat)
    N = len(th)
    vd = L.vp_sampler_desc(N, 1, t, th, c, 0.9, w)
    shape = (B, 1, H, W)
    h, init = fx.randn("exact/vp/h", *shape), fx.randn("exact/vp/init", *shape)
    steps = E.draws64("vp", N, shape)
    dev_steps = torch.stack(steps).cuda()
    P, packed = (n.P0, n.packed0) if zero else (n.P, n.packed)
    net = orc.self_cond_net(P, n.cfg)
    _both(lambda last: n.plan.vp_sample(packed, vd, h.cuda(), init.cuda(), dev_steps, return_last=last),
          lambda last: orc.sample_vp_heun(net, h, t, th, c, init, steps, S_noise=0.9, w=w, return_last=last),
          f"vp_heun_sample {case}")


def test_vp_heun_guided_swe(wide):
    L, n = wide.L, wide
    gd, guide = _guidance(L)
    t, th, c = E.vp_schedule(E.ddpm_tables()[0], *E.VP_GUIDED_SIGMAS)
    N = len(th)
    vd = L.vp_sampler_desc(N, 1, t, th, c, 0.9, 0.0)
    shape = (B, 1, H, W)
    h, init = _water("vpg", *shape), fx.randn("exact/vpg/init", *shape)
    steps = E.draws64("vpg", N, shape)
    dev_steps = torch.stack(steps).cuda()
    net = orc.self_cond_net(n.P, n.cfg)
    xs = _both(lambda last: n.plan.vp_sample(n.packed, vd, h.cuda(), init.cuda(), dev_steps, return_last=last, guidance=gd),
               lambda last: orc.sample_vp_heun(net, h, t, th, c, init, steps, S_noise=0.9, w=0.0, guidance=guide, return_last=last),
               "vp_heun_sample_guided swe")
    with torch.no_grad(), E.ieee_sqrt():
        plain = orc.sample_vp_heun(net, h, t, th, c, init, steps, S_noise=0.9, w=0.0, return_last=False)
    assert torch.isfinite(xs).all() and not torch.equal(xs[:, 1], plain[:, 1])


# ---- 3. mcedm_cond_ddim_sample -------------------------------------------------------------------------------------------------
def _ddim_desc(L, N, skip, eta, w, aext):
    sp = types.SimpleNamespace(timesteps=N, skip_type=skip, eta=eta, w=w)
    dd = L.cond_ddim_desc(sp, aext, 1, True)
    seq = L.ddim_timesteps(1000, N, skip)
    assert seq == ddo.ddim_sequence(1000, ddo.DdimParams(timesteps=N, skip_type=skip))
    return dd, seq


@pytest.mark.parametrize("skip,N", [("uniform", 7), ("quad", 5)])
@pytest.mark.parametrize("eta", [0.0, 0.5])
def test_cond_ddim(wide, eta, skip, N):
    """PlCondDdim.sample, fp32: self_cond 1, w 0.5; uniform with 7 timesteps walks 8 entries (1000 // 7 = 142)."""
    L, n = wide.L, wide
    aext = E.ddpm_tables()[1]
    dd, seq = _ddim_desc(L, N, skip, eta, 0.5, aext)
    assert len(seq) == (8 if skip == "uniform" else 5)
    shape = (B, 1, H, W)
    h, init = fx.randn("exact/ddim/h", *shape), fx.randn("exact/ddim/init", *shape)
    draws = E.uniform32("ddim", len(seq), shape)
    dev_draws = torch.stack(draws).cuda() if eta else None
    net = orc.self_cond_net(n.P, n.cfg)
    xs, x0 = _both(lambda last: n.plan.cond_ddim_sample(n.packed, dd, h.cuda(), init.cuda(), dev_draws, return_last=last),
                   lambda last: orc.sample_cond_ddim(net, h, aext, seq, init, eta=eta, w=0.5, eta_noise=draws, return_last=last),
                   f"cond_ddim_sample {skip} eta={eta}")
    assert tuple(xs.shape) == (B, len(seq) + 1, H, W, 1) and tuple(x0.shape) == (B, len(seq), H, W, 1)
    assert torch.equal(xs[:, 0], init.permute(0, 2, 3, 1))


# ---- 4. the joint DDPM model: mcedm_repaint_sample, mcedm_ddim_repaint_sample ----------------------------------------------------
def _joint_inputs(tag):
    h, u = fx.randn(f"exact/{tag}/h", B, R, R, 1), fx.randn(f"exact/{tag}/u", B, R, R, 1)
    return h, u, torch.cat([h, u], dim=-1).permute(0, 3, 1, 2).contiguous(), fx.randn(f"exact/{tag}/init", B, 2, R, R)


def _known(last, h, u, nth, ntu):
    """Known rows of the last slot equal the clean data."""
    known = torch.ones(B, R, R, 2, dtype=torch.bool)
    known[:, nth:, :, 0] = False
    known[:, ntu:, :, 1] = False
    assert torch.equal(last[known], torch.cat([h, u], dim=-1).to(last.dtype)[known])
    assert not torch.equal(last[~known], torch.cat([h, u], dim=-1).to(last.dtype)[~known])


def test_repaint(d_joint):
    """PlDdim.sample_edm: n_repeat 3, rows [0, 3) of h and [0, 5) of u known, a window that cuts the churn on both sides."""
    L, n = d_joint.L, d_joint
    sp = ddo.RepaintParams(**E.REPAINT)
    steps_table, aext = E.ddpm_tables(n.cfg)
    with E.ieee_sqrt():                        # the table sample_edm_repaint builds for itself is the one the library is given
        assert torch.equal(ddo.edm_steps_of(ddo.betas_of(n.cfg)), steps_table)
    rd, keep = L.repaint_desc(sp, steps_table, aext, 1, 1)
    t = L.repaint_schedule(rd)
    smin, smax = max(sp.sigma_min, float(steps_table[-1])), min(sp.sigma_max, float(steps_table[0]))
    idx = torch.arange(sp.timesteps, dtype=torch.float64)
    want = ddo.round_sigma(steps_table, (smax ** (1 / sp.rho) + idx / (sp.timesteps - 1) * (smin ** (1 / sp.rho) - smax ** (1 / sp.rho))) ** sp.rho)
    assert E.within_ulps(t, want.tolist() + [0.0]) and t == want.tolist() + [0.0]      # rounded onto the table: the same entries
    on = E.churns(t, sp.S_churn, sp.S_min, sp.S_max)
    assert any(on) and not on[0] and not on[-1]
    h, u, hu, init = _joint_inputs("repaint")
    shape = (B, 2, R, R)
    steps = E.draws64("repaint", sp.timesteps, shape)
    reps = [E.draws64(f"repaint/rep{i}", sp.n_repeat - 1, shape) for i in range(sp.timesteps)]
    dev_steps, dev_reps = torch.stack(steps).cuda(), torch.stack([torch.stack(r) for r in reps]).cuda()
    xs = _both(lambda last: n.plan.repaint_sample(n.packed, rd, hu.cuda(), init.cuda(), dev_steps, dev_reps, return_last=last),
               lambda last: ddo.sample_edm_repaint(n.P, n.cfg, hu, sp, init, steps, reps, return_last=last),
               "repaint_sample")
    _known(xs[:, -1], h, u, sp.n_time_h, sp.n_time_u)


def test_ddim_repaint(d_joint):
    """PlDdim.sample_with_repeat: eta 0.5, n_repeat 2, both fields partly known."""
    L, n = d_joint.L, d_joint
    sp = ddo.DdimParams(**E.DDIM_REPAINT)
    aext = E.ddpm_tables(n.cfg)[1]
    dd, keep = L.ddim_desc(sp, aext, 1, 1, True)
    seq = L.ddim_timesteps(n.cfg.num_timesteps, sp.timesteps, sp.skip_type)
    assert seq == ddo.ddim_sequence(n.cfg.num_timesteps, sp)
    h, u, hu, init = _joint_inputs("ddimr")
    draws = E.uniform32("ddimr", len(seq), (B, 2, R, R))
    dev_draws = torch.stack(draws).cuda()
    xs, x0 = _both(lambda last: n.plan.ddim_repaint_sample(n.packed, dd, hu.cuda(), init.cuda(), dev_draws, return_last=last),
                   lambda last: ddo.sample_with_repeat(n.P, n.cfg, hu, sp, init, draws, return_last=last),
                   "ddim_repaint_sample")
    _known(x0[:, -1], h, u, sp.n_time_h, sp.n_time_u)


# ---- 5. the single-task entries of the DDPM U-Net: their loops are shared, their denoiser finishing code is not ------------------
def test_ddpm_vp_heun(d_head):
    """mcedm_ddpm_vp_heun_sample: launch_vp_cfg_finish behind the cond_enc head (cond enters unscaled)."""
    L, n = d_head.L, d_head
    t, th, c = E.vp_schedule(E.ddpm_tables(n.cfg)[0], *E.VP_SIGMAS)
    N = len(th)
    vd = L.vp_sampler_desc(N, 1, t, th, c, 0.9, 0.5)
    shape = (B, 1, R, R)
    h, init = fx.randn("exact/dvp/h", *shape), fx.randn("exact/dvp/init", *shape)
    steps = E.draws64("dvp", N, shape)
    dev_steps = torch.stack(steps).cuda()
    net = E.ddpm_net(n.P, n.cfg)
    _both(lambda last: n.plan.vp_sample(n.packed, vd, h.cuda(), init.cuda(), dev_steps, return_last=last),
          lambda last: orc.sample_vp_heun(net, h, t, th, c, init, steps, S_noise=0.9, w=0.5, return_last=last, scale_cond=False),
          "ddpm_vp_heun_sample")


def test_ddpm_cond_ddim(d_head):
    L, n = d_head.L, d_head
    aext = E.ddpm_tables(n.cfg)[1]
    dd, seq = _ddim_desc(L, 5, "quad", 0.5, 0.5, aext)
    shape = (B, 1, R, R)
    h, init = fx.randn("exact/dddim/h", *shape), fx.randn("exact/dddim/init", *shape)
    draws = E.uniform32("dddim", len(seq), shape)
    dev_draws = torch.stack(draws).cuda()
    net = E.ddpm_net(n.P, n.cfg)
    _both(lambda last: n.plan.cond_ddim_sample(n.packed, dd, h.cuda(), init.cuda(), dev_draws, return_last=last),
          lambda last: orc.sample_cond_ddim(net, h, aext, seq, init, eta=0.5, w=0.5, eta_noise=draws, return_last=last),
          "ddpm_cond_ddim_sample")


@pytest.mark.parametrize("case", ["window", "one_step"])
def test_ddpm_edm_heun(d_cat, case):
    """mcedm_ddpm_edm_heun_sample: launch_edm_cfg_finish with c_skip / c_out formed on the host, sigma_data 0.5, w 0.5;
    one_step: timesteps == 1, Euler only."""
    L, n = d_cat.L, d_cat
    sch = E.EDM_SCHED if case == "window" else E.EDM_ONE_STEP
    t, th, c = E.edm_schedule(**sch)
    N = len(th)
    vd = L.vp_sampler_desc(N, 1, t, th, c, 0.9, 0.5)
    sp = orc.SamplerParams(timesteps=N, S_churn=sch["S_churn"], S_min=sch["S_min"], S_max=sch["S_max"], S_noise=0.9, w=0.5)
    shape = (B, 1, R, R)
    h, init = fx.randn("exact/dedm/h", *shape), fx.randn("exact/dedm/init", *shape)
    steps = E.draws64("dedm", N, shape)
    dev_steps = torch.stack(steps).cuda()
    net = E.ddpm_cat_net(n.P, n.cfg)
    _both(lambda last: n.plan.edm_sample(n.packed, vd, h.cuda(), init.cuda(), dev_steps, return_last=last, sigma_data=E.SIGMA_DATA),
          lambda last: orc.sample_edm_cond(None, None, h, sp, init, steps, return_last=last, sigma_data=E.SIGMA_DATA, t_steps=t, net=net),
          f"ddpm_edm_heun_sample {case}")
