"""CPU groundwork of tests/test_hip_sampler_exact.py: both oracle networks return the bias of their last convolution exactly on
constant parameters, the two sampler loops added to the oracle for PlCondDdim (sample_vp_heun, sample_cond_ddim) reproduce the
reference's recorded runs with real weights, the new optional arguments of the EDM loops change nothing by default, and every
schedule the device cases use has a step that churns and one that does not."""
import numpy as np
import pytest
import torch

from oracle import ddpm_oracle as ddo
from oracle import fixtures as fx
from oracle import mcedm_oracle as orc
from tests import _cond_guided as G
from tests import _sampler_exact as E
from tests._tol import close_per_entry


# ---- 1. F == bias ------------------------------------------------------------------------------------------------------------
def _expect(bias, n, h, w):
    return torch.tensor(list(bias), dtype=torch.float32).view(1, -1, 1, 1).expand(n, -1, h, w)


@pytest.mark.parametrize("cfg", [E.CFG_JOINT, E.CFG_SINGLE, E.CFG_WIDE], ids=["joint", "single", "wide"])
def test_adm_network_returns_its_last_bias(cfg):
    """unet_forward on constant parameters, with and without cond, at large inputs and across the noise labels: no NaN from the
    zero-variance GroupNorms, no trace of the input."""
    P = E.constant_params(orc.make_params, cfg, E.bias_of(cfg))
    x = fx.randn("exact/cpu/adm/x", E.B, cfg.in_channels, E.H, E.W) * 80.0
    cond = fx.randn("exact/cpu/adm/cond", E.B, cfg.cond_channels, E.H, E.W)
    want = _expect(E.bias_of(cfg), E.B, E.H, E.W)
    with torch.no_grad():
        for labels in (torch.tensor([1.0955]), torch.tensor([-1.5536, 0.0, 999.0])):
            for c in (cond, None):
                assert torch.equal(orc.unet_forward(P, cfg, x, labels, c), want)
        if cfg is E.CFG_WIDE:                       # the self-conditioning convention of PlCondDdim's network
            net = orc.self_cond_net(P, cfg)
            for c, sc in ((cond[:, :1], x), (None, x), (cond[:, :1], None)):
                assert torch.equal(net(x, torch.tensor([500.0]), c, sc), want)
        P0 = E.constant_params(orc.make_params, cfg, E.bias_of(cfg, zero=True))
        assert torch.equal(orc.unet_forward(P0, cfg, x, torch.tensor([0.3]), cond), torch.zeros_like(want))


@pytest.mark.parametrize("cfg", [E.CFG_D_JOINT, E.CFG_D_HEAD, E.CFG_D_CAT], ids=["joint", "head", "cat"])
def test_ddpm_network_returns_its_last_bias(cfg):
    P = E.constant_params(ddo.make_params, cfg, E.bias_of(cfg))
    x = fx.randn("exact/cpu/ddpm/x", E.B, cfg.in_channels, E.R, E.R) * 80.0
    xsc = fx.randn("exact/cpu/ddpm/xsc", E.B, cfg.in_channels, E.R, E.R) if cfg.self_cond else None
    cond = fx.randn("exact/cpu/ddpm/cond", E.B, cfg.cond_channels, E.R, E.R) if cfg.cond_channels else None
    want = _expect(E.bias_of(cfg), E.B, E.R, E.R)
    with torch.no_grad():
        for t in (0.0, 937.0):
            for c in (cond, None):
                for s in (xsc, None):
                    assert torch.equal(ddo.model_forward(P, cfg, x, torch.full((E.B,), t), x_self_cond=s, cond=c), want)


def test_constant_net_is_what_the_networks_compute():
    """const_net (the network skipped, for the case past the grid cap) against the oracle network on the same call."""
    cfg = E.CFG_JOINT
    P = E.constant_params(orc.make_params, cfg, E.bias_of(cfg))
    x = fx.randn("exact/cpu/const/x", 2, 2, E.H, E.W)
    with torch.no_grad():
        assert torch.equal(E.const_net(E.bias_of(cfg))(x, torch.tensor([0.1]), None), E.adm_net(P, cfg)(x, torch.tensor([0.1]), None))


# ---- 2. the new oracle loops against the reference's recorded runs ---------------------------------------------------------------
def _wide_params(golden):
    return orc.make_params(E.CFG_WIDE, int(golden("cond_ddim.npz")["seed"]))


def _alphas_ext():
    return ddo.alphas_ext_of(ddo.betas_of(ddo.DdpmConfig()))


DDIM_CASES = {"uni": (10, "uniform", 0.0, 0.0), "cfg_eta": (10, "uniform", 0.5, 0.5), "quad": (8, "quad", 0.0, 0.0),
              "uneven": (7, "uniform", 0.0, 0.0)}       # the CASES of tools/make_golden_cond_ddim_sample.py


@pytest.mark.parametrize("tag", list(DDIM_CASES))
def test_ddim_loop_reproduces_the_reference_runs(golden, tag):
    """sample_cond_ddim on the oracle network with the weights and draws of tests/golden/cond_ddim_sample.npz, at the bar of
    tests/test_hip_cond_ddim_sample.py (rtol 1e-4, atol 1e-5 x max|slot|)."""
    g = golden("cond_ddim_sample.npz")
    N, skip, eta, w = DDIM_CASES[tag]
    P = orc.make_params(E.CFG_WIDE, int(g["seed"]))
    Bq, Hq, Wq = 3, 32, 32
    h = fx.randn("cddim/ddim/h", Bq, Hq, Wq, 1).permute(0, 3, 1, 2)
    un = fx.randn("cddim/ddim/u_noise", Bq, Hq, Wq, 1).permute(0, 3, 1, 2)
    seq = ddo.ddim_sequence(1000, ddo.DdimParams(timesteps=N, skip_type=skip))
    draws = [torch.from_numpy(((fx.uniform(f"cddim/ddim/{tag}/eta{k}", Bq, 1, Hq, Wq) + 1.0) * 0.5).astype(np.float32)) for k in range(len(seq))]
    with torch.no_grad():
        xs, x0 = orc.sample_cond_ddim(orc.self_cond_net(P, E.CFG_WIDE), h, _alphas_ext(), seq, un, eta=eta, w=w, eta_noise=draws,
                                      return_last=False)
        xs_last, x0_last = orc.sample_cond_ddim(orc.self_cond_net(P, E.CFG_WIDE), h, _alphas_ext(), seq, un, eta=eta, w=w,
                                                eta_noise=draws, return_last=True)
    assert xs.dtype == x0.dtype == torch.float32
    print(f"{tag}: xs worst err / bar {close_per_entry(xs, g[f'{tag}::xs'], what=f'{tag} xs'):.4f}, "
          f"x0_preds {close_per_entry(x0, g[f'{tag}::x0_preds'], what=f'{tag} x0_preds'):.4f}")
    assert torch.equal(xs_last[:, 0], xs[:, -1]) and torch.equal(x0_last[:, 0], x0[:, -1])


def _guided_vp_schedule(tag):
    """The schedule PlCondDdim.sample_edm derives from the sampler block of tests/_cond_guided.py (models/ddim.py:1543-1553, 1566)."""
    sp = G.sampler_dict(tag)
    steps = ddo.edm_steps_of(ddo.betas_of(ddo.DdpmConfig()))
    N, rho = sp["timesteps"], float(sp["rho"])
    smin, smax = max(sp["sigma_min"], float(steps[-1])), min(sp["sigma_max"], float(steps[0]))
    idx = torch.arange(N, dtype=torch.float64)
    t = (smax ** (1 / rho) + idx / (N - 1) * (smin ** (1 / rho) - smax ** (1 / rho))) ** rho
    t = torch.cat([ddo.round_sigma(steps, t), torch.zeros_like(t[:1])])
    cn = lambda s: float(999 - int(ddo.round_sigma(steps, s.to(torch.float32).reshape(1), return_index=True)[0]))      # noqa: E731
    t_hat, c_noise = [], []
    for i in range(N):
        gamma = min(sp["S_churn"] / N, np.sqrt(2) - 1) if sp["S_min"] <= t[i] <= float(sp["S_max"]) else 0
        th = ddo.round_sigma(steps, t[i] + gamma * t[i])
        t_hat.append(float(th))
        c_noise += [cn(th), cn(t[i + 1]) if i < N - 1 else 0.0]
    return t, t_hat, c_noise, sp


@pytest.mark.parametrize("tag", ["vp", "vp_churn_cfg"])
def test_vp_heun_loop_reproduces_the_reference_runs(golden, tag):
    """sample_vp_heun on the oracle network against tests/golden/cond_guided.npz: the guided trajectory on its recorded prefix and
    the unguided state of the same slot, at the bar of tests/test_hip_cond_guided.py."""
    g = golden(G.GOLDEN["adm"])
    key = f"adm::{tag}"
    n = int(g[f"{key}::slots"])
    P = _wide_params(golden)
    h, un = (v.permute(0, 3, 1, 2) for v in G.inputs())
    t, t_hat, c_noise, sp = _guided_vp_schedule(tag)
    net = orc.self_cond_net(P, E.CFG_WIDE)
    st = fx.STEP_NORM_STATS
    guide = lambda hh, dd: orc.guidance_dx_cond("swe_per", hh, dd, st)      # noqa: E731
    draws = G.step_draws(tag)
    with torch.no_grad():
        xs = orc.sample_vp_heun(net, h, t, t_hat, c_noise, un, draws, S_noise=sp["S_noise"], w=sp["w"], guidance=guide,
                                return_last=False)
        plain = orc.sample_vp_heun(net, h, t, t_hat, c_noise, un, draws, S_noise=sp["S_noise"], w=sp["w"], return_last=False)
    assert xs.dtype == torch.float64 and tuple(xs.shape) == tuple(g[f"{key}::xs"].shape)
    err = close_per_entry(xs[:, :n + 1], g[f"{key}::xs"][:, :n + 1], what=f"{key} xs")
    perr = close_per_entry(plain[:, n:n + 1], g[f"{key}::unguided_last"], what=f"{key} unguided")
    print(f"{key}: {n} steps, worst err / bar {err:.4f} (unguided {perr:.4f})")


# ---- 3. the optional arguments of the EDM loops leave their defaults alone ----------------------------------------------------------
def test_edm_loops_defaults_are_unchanged_and_the_new_arguments_act():
    cfg = E.CFG_JOINT
    P = E.constant_params(orc.make_params, cfg, E.bias_of(cfg))
    cond = fx.randn("exact/cpu/edm/cond", 2, 2, E.H, E.W)
    mask = E.fractional_mask("cpu/edm", (2, 2, E.H, E.W))
    init = fx.randn("exact/cpu/edm/init", 2, 2, E.H, E.W)
    sp = orc.SamplerParams(timesteps=4)
    with torch.no_grad():
        base = orc.sample_edm(P, cfg, cond, mask, sp, init, return_last=False)
        trace = []
        same = orc.sample_edm(P, cfg, cond, mask, sp, init, return_last=False, sigma_data=orc.SIGMA_DATA,
                              t_steps=orc.edm_t_steps(4, sp.sigma_min, sp.sigma_max, sp.rho), net=E.const_net(E.bias_of(cfg)), trace=trace)
        other = orc.sample_edm(P, cfg, cond, mask, sp, init, return_last=False, sigma_data=E.SIGMA_DATA)
    assert torch.equal(base, same) and not torch.equal(base[:, 1:], other[:, 1:])
    assert len(trace) == 4 and "d_prime" in trace[0] and "d_prime" not in trace[3]
    for i, st in enumerate(trace):
        assert torch.equal(st["x_next"].permute(0, 2, 3, 1), base[:, i + 1])
    Pc = E.constant_params(orc.make_params, E.CFG_SINGLE, E.bias_of(E.CFG_SINGLE))
    with torch.no_grad():
        a = orc.sample_edm_cond(Pc, E.CFG_SINGLE, cond[:, :1], sp, init[:, :1])
        b = orc.sample_edm_cond(Pc, E.CFG_SINGLE, cond[:, :1], sp, init[:, :1], net=E.const_net(E.bias_of(E.CFG_SINGLE)), trace=[])
    assert torch.equal(a, b)


def test_one_ulp_in_the_network_output_moves_the_trajectory():
    """The bit comparison is as sharp as it claims: F one fp32 ulp up changes the last slot of the window case."""
    cfg = E.CFG_JOINT
    shape = (E.B, 2, E.H, E.W)
    cond, init = fx.randn("exact/masked/cond", *shape), fx.randn("exact/masked/init", *shape)
    mask = E.fractional_mask("masked", shape)
    sp = orc.SamplerParams(**E.WINDOW)
    steps = E.draws64("masked", sp.timesteps, shape)
    b = torch.tensor(E.bias_of(cfg))
    up = torch.nextafter(b, b + 1)
    with torch.no_grad(), E.ieee_sqrt():
        a = orc.sample_edm(None, cfg, cond, mask, sp, init, steps, sigma_data=E.SIGMA_DATA, net=E.const_net(b.tolist()))
        c = orc.sample_edm(None, cfg, cond, mask, sp, init, steps, sigma_data=E.SIGMA_DATA, net=E.const_net(up.tolist()))
    moved = (a != c) & (mask != 0).permute(0, 2, 3, 1).unsqueeze(1)
    assert float(moved.double().mean()) > 0.25 and 0 < E.ulps_apart(a, c)
    assert torch.equal(a[(mask == 0).permute(0, 2, 3, 1).unsqueeze(1)], c[(mask == 0).permute(0, 2, 3, 1).unsqueeze(1)])


# ---- 4. the schedules of the device cases -----------------------------------------------------------------------------------------
def test_window_schedule_churns_in_the_middle_only():
    w = E.WINDOW
    t = orc.edm_t_steps(w["timesteps"], 0.002, 80.0, w["rho"])
    assert [float(v) for v in t[:-1]] == pytest.approx([80.0, 30.39, 9.14, 1.88, 0.182, 0.002], rel=5e-3)
    on = E.churns(t, w["S_churn"], w["S_min"], w["S_max"])
    assert on == E.WINDOW_CHURNS and not on[0] and not on[-1] and any(on)      # a step that does not churn on each side
    assert min(w["S_churn"] / w["timesteps"], np.sqrt(2) - 1) == np.sqrt(2) - 1


def test_rounded_schedules_have_a_churning_and_a_plain_step():
    steps, _ = E.ddpm_tables()
    for t, th, c in (E.vp_schedule(steps, *E.VP_SIGMAS), E.vp_schedule(steps, *E.VP_GUIDED_SIGMAS), E.edm_schedule(**E.EDM_SCHED)):
        moved = [th[i] != t[i] for i in range(len(th))]
        assert any(moved) and not all(moved) and all(th[i] >= t[i] > 0 for i in range(len(th))) and len(c) == 2 * len(th)
        assert c[-1] == 0.0
    t, th, c = E.vp_schedule(steps, *E.ONE_STEP)
    assert len(t) == 2 and th[0] > t[0] > 0 and t[1] == 0.0
    t, th, c = E.edm_schedule(**E.EDM_ONE_STEP)
    assert len(t) == 2 and th[0] > t[0] > 0 and t[1] == 0.0
    # RePaint on the rounded table: the window cuts the churn on both sides
    sp = ddo.RepaintParams(**E.REPAINT)
    smin, smax = max(sp.sigma_min, float(steps[-1])), min(sp.sigma_max, float(steps[0]))
    idx = torch.arange(sp.timesteps, dtype=torch.float64)
    t = ddo.round_sigma(steps, (smax ** (1 / sp.rho) + idx / (sp.timesteps - 1) * (smin ** (1 / sp.rho) - smax ** (1 / sp.rho))) ** sp.rho)
    on = E.churns(list(t) + [0.0], sp.S_churn, sp.S_min, sp.S_max)
    assert any(on) and not on[0] and not on[-1], on
    for i, v in enumerate(t):                # a churning step really moves on the table; a plain one stays
        th = ddo.round_sigma(steps, v + (np.sqrt(2) - 1 if on[i] else 0.0) * v)
        assert (float(th) > float(v)) == on[i]


def test_the_odd_guidance_weight_tells_the_two_roundings_apart():
    w = E.W_ODD
    assert np.float32(w + 1.0) != np.float32(np.float32(w) + np.float32(1.0))
    assert float(torch.tensor([1.0]) * (w + 1)) == float(np.float32(w + 1.0))      # what (w + 1) * F multiplies by
    f = np.float32
    for b in E.BIAS:                         # and the blended constant (w + 1) F - w F differs with it, in both channels
        blend = lambda w1: f(f(w1 * f(b)) - f(f(w) * f(b)))      # noqa: E731
        assert blend(f(w + 1.0)) != blend(f(f(w) + f(1.0)))


def test_ulp_distance_counts_representable_numbers():
    a = torch.tensor([1.0, -1.0, 0.0, 247.0], dtype=torch.float64)
    assert E.ulps_apart(a, a) == 0
    assert E.ulps_apart(torch.nextafter(a, torch.full_like(a, 1e9)), a) == 1
    assert E.ulps_apart(torch.tensor([-0.0]), torch.tensor([0.0])) == 0
    b = torch.tensor([0.37, -1.21])
    assert E.ulps_apart(torch.nextafter(torch.nextafter(b, -b * 9), -b * 9), b) == 2
    assert E.within_ulps([80.0, 1.0], [float(np.nextafter(80.0, 90.0)), 1.0]) and not E.within_ulps([80.0], [80.0 + 1e-12])


def test_ieee_sqrt_is_correctly_rounded_and_scoped():
    """Inside the context the square root of a CPU tensor is the correctly rounded one (fp32: the fp64 root rounded once more --
    53 >= 2 * 24 + 2 bits make the double rounding harmless); outside it torch's own is back."""
    v = torch.from_numpy((np.random.default_rng(5).random(100000) * 1000).astype(np.float32))
    real = torch.Tensor.sqrt
    with E.ieee_sqrt():
        got, got0, got64 = v.sqrt(), torch.sqrt(v[7]), v.double().sqrt()
        assert got.dtype == torch.float32 and got0.shape == () and got64.dtype == torch.float64
        strided = v.view(100, 1000)[:, ::3].sqrt()
    want = torch.from_numpy(np.sqrt(v.numpy().astype(np.float64)).astype(np.float32))
    assert torch.equal(got, want) and got0 == want[7] and torch.equal(strided, want.view(100, 1000)[:, ::3])
    assert torch.equal(got64, torch.from_numpy(np.sqrt(v.numpy().astype(np.float64))))
    assert torch.Tensor.sqrt is real and float((v.sqrt() - want).abs().max()) <= float(torch.finfo(torch.float32).eps * 32)
