"""GPU: device-side noise and graph replay of the remaining samplers.

  * the uniform generator (mcedm_uniform_fill) bit for bit against a NumPy restatement of Philox4x32-10, which is first held to
    the Random123 known-answer vectors; its moments, and its independence of the normal stream of the same seed;
  * the conditional DDIM step kernel with (rng_seed, draw) == the same kernel fed uniform_fill's tensor, on the four shapes of
    tests/test_hip_cond_ddim_sample.py::test_step_kernel_against_fp64, and behind a pointer that is not 16-byte aligned;
  * the four `_rng` sampler entries == their siblings fed the materialised draws;
  * the four module calls under noise_source = "device" (reproducible from torch's seed, no noise tensor, one graph, graph ==
    eager) and, for the two calls that gained graph replay, replay == eager launches under "torch"."""
import math

import numpy as np
import pytest
import torch

from oracle import ddpm_oracle as dorc
from oracle import fixtures as fx
from oracle import mcedm_oracle as orc
from tests.test_cond_ddim_sample_cpu import alphas_ext, sparams
from tests.test_hip_cond_ddim import B, H, W, make_module
from tests.test_hip_cond_edm import cond_hparams
from tests.test_hip_ddpm import hparams as ddpm_hparams
from tests.test_hip_module import wrap

pytestmark = pytest.mark.gpu

MASK = np.uint64(0xFFFFFFFF)


# ---- Philox4x32-10 (Salmon et al. 2011), restated ---------------------------------------------------------------------
def philox4x32_10(ctr, key):
    """ctr [n, 4] uint32 counters, key (k0, k1) -> [n, 4] uint32 words."""
    c = [ctr[:, i].astype(np.uint64) for i in range(4)]
    k0, k1 = np.uint64(key[0]), np.uint64(key[1])
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & MASK]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & MASK, (k1 + np.uint64(0xBB67AE85)) & MASK
    return np.stack(c, axis=1).astype(np.uint32)


def uniform_ref(seed, draw, n):
    """Element e of draw d: word e % 4 of the block at counter (lo32(e / 4), hi32(e / 4), lo32(d), hi32(d) | 2^31), as
    (word >> 8) * 2^-24."""
    e = np.arange(n, dtype=np.uint64)
    g = e >> np.uint64(2)
    d = np.uint64(draw)
    ctr = np.stack([g & MASK, g >> np.uint64(32), np.full(n, d & MASK), np.full(n, (d >> np.uint64(32)) | np.uint64(0x80000000))],
                   axis=1).astype(np.uint32)
    words = philox4x32_10(ctr, (seed & 0xFFFFFFFF, seed >> 32))[np.arange(n), (e & np.uint64(3)).astype(np.int64)]
    return (words >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)


def test_philox_restatement_known_answers():
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in kat:
        got = philox4x32_10(np.array([ctr], dtype=np.uint32), key)[0]
        assert tuple(int(v) for v in got) == want, [hex(int(v)) for v in got]


@pytest.fixture(scope="module")
def L():
    import mcedm_amd  # noqa: F401
    from mcedm_amd import lib
    return lib


def dev_seed(v):
    return torch.tensor([v], dtype=torch.int64, device="cuda")


@pytest.mark.parametrize("draw", [0, 1, 2 ** 40 + 3])
@pytest.mark.parametrize("n", [1, 5, 4099])
def test_uniform_fill_bit_for_bit(L, n, draw):
    test_philox_restatement_known_answers()
    seed = 0x123456789ABCDE
    want = uniform_ref(seed, draw, n)
    got = L.uniform_fill(torch.full((n,), -1.0, device="cuda"), dev_seed(seed), draw).cpu().numpy()
    assert np.array_equal(got, want)
    buf = torch.full((n + 2,), -1.0, device="cuda")                       # one element past a 16-byte boundary
    off = L.uniform_fill(buf[1:n + 1], dev_seed(seed), draw)
    assert off.data_ptr() % 16 == 4 and np.array_equal(off.cpu().numpy(), want)
    assert float(buf[0]) == -1.0 and float(buf[n + 1]) == -1.0           # nothing outside the n elements
    assert bool((got >= 0).all()) and bool((got < 1).all())
    assert np.array_equal(got * np.float32(2.0 ** 24), np.floor(got * np.float32(2.0 ** 24)))      # multiples of 2^-24


def test_uniform_moments_and_independence(L):
    n = 1 << 18
    seed = dev_seed(77)
    u = torch.stack([L.uniform_fill(torch.empty(n, device="cuda"), seed, d) for d in range(4)]).double()
    z = torch.stack([L.normal_fill(torch.empty(n, dtype=torch.float64, device="cuda"), seed, d) for d in range(4)])
    for d in range(4):
        mean, var = float(u[d].mean()), float(u[d].var(unbiased=False))
        print(f"draw {d}: mean - 1/2 = {mean - 0.5:+.3e} (5 sigma {5 / math.sqrt(12 * n):.3e}), "
              f"var - 1/12 = {var - 1 / 12:+.3e} (5 sigma {5 / math.sqrt(180 * n):.3e})")
        assert abs(mean - 0.5) < 5 / math.sqrt(12 * n)
        assert abs(var - 1 / 12) < 5 / math.sqrt(180 * n)
    c = torch.corrcoef(torch.cat([u, z]))
    off = c[:4, :4] - torch.eye(4, device="cuda", dtype=torch.float64)
    print(f"max |corr| between draws {float(off.abs().max()):.3e}, with the normal stream of the same (seed, draw) "
          f"{float(c[:4, 4:].diagonal().abs().max()):.3e} (bound {5 / math.sqrt(n):.3e})")
    assert float(off.abs().max()) < 5 / math.sqrt(n)
    assert float(c[:4, 4:].diagonal().abs().max()) < 5 / math.sqrt(n)


# ---- the step kernel ---------------------------------------------------------------------------------------------------
def _f32(v):
    return float(np.float32(v))


def _step(L, shape, guided, xt, F, Fu, **noise):
    Bq, Cq, Hq, Wq = shape
    tag = "x".join(map(str, shape))
    cc, Cp, T = 2, 2 + Cq + 1, 3
    cond = fx.randn(f"cddim/step/{tag}/cond", Bq, Cp, Hq, Wq).cuda()
    condp, condu = cond.clone(), (cond * 2).clone()
    xs = torch.full((Bq, T + 1, Hq, Wq, Cq), 7.0, device="cuda")
    x0s = torch.full((Bq, T, Hq, Wq, Cq), 7.0, device="cuda")
    s0, s1, sa = _f32(np.sqrt(np.float32(0.3))), _f32(np.sqrt(np.float32(0.7))), _f32(np.sqrt(np.float32(0.55)))
    xn = L.op_ddim_cond_step(xt, F, s0, s1, sa, _f32(0.6), Fu=Fu if guided else None, w=0.5, c1=_f32(0.4), condp=condp,
                             condp_u=condu if guided else None, cond_channels=cc, xs=xs, t_xs=2, x0s=x0s, t_x0=1, **noise)
    return xn, condp, condu, xs, x0s


@pytest.mark.parametrize("guided", [False, True])
@pytest.mark.parametrize("shape", [(3, 1, 32, 32), (1, 1, 5, 7), (2, 2, 6, 6), (2, 3, 5, 7)])
def test_step_kernel_generates_what_uniform_fill_writes(L, shape, guided):
    tag = "x".join(map(str, shape))
    xt, F, Fu = (fx.randn(f"cddim/step/{tag}/{k}", *shape).cuda() for k in ("xt", "F", "Fu"))
    seed, draw = dev_seed(991), 5
    nz = L.uniform_fill(torch.empty(shape, device="cuda"), seed, draw)
    want = _step(L, shape, guided, xt, F, Fu, noise=nz)
    got = _step(L, shape, guided, xt, F, Fu, rng_seed=seed, draw=draw)
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    assert not torch.equal(got[0], _step(L, shape, guided, xt, F, Fu, rng_seed=seed, draw=draw + 1)[0])
    # xt one element past a 16-byte boundary: every element takes the scalar path and gets the same value
    buf = torch.empty(xt.numel() + 1, device="cuda")
    buf[1:].copy_(xt.reshape(-1))
    xt_off = buf[1:].view(shape)
    assert xt_off.data_ptr() % 16 == 4
    for a, b in zip(_step(L, shape, guided, xt_off, F, Fu, rng_seed=seed, draw=draw), want):
        assert torch.equal(a, b)
    with pytest.raises(RuntimeError, match="not both"):
        _step(L, shape, guided, xt, F, Fu, noise=nz, rng_seed=seed)


# ---- samplers against the materialised draws -----------------------------------------------------------------------------
@pytest.mark.parametrize("return_last", [False, True])
@pytest.mark.parametrize("timesteps,S", [(4, 4), (7, 8)])
def test_cond_ddim_sample_rng_equals_the_materialised_draws(L, golden, timesteps, S, return_last):
    m = make_module(golden, **dict(sparams(timesteps=timesteps, eta=0.5, w=0.5)))
    net = m.ema_model.ma_model
    dd = L.cond_ddim_desc(m.sparams, alphas_ext(), 1, True)
    assert len(L.ddim_timesteps(1000, timesteps, "uniform")) == S
    h = fx.randn("cddim/ddim/h", B, H, W, 1).permute(0, 3, 1, 2).contiguous().cuda()
    un = fx.randn("cddim/ddim/u_noise", B, H, W, 1).permute(0, 3, 1, 2).contiguous().cuda()
    seed = dev_seed(4242)
    with torch.no_grad():
        pk = net.packed_weights()
        eta_noise = torch.stack([L.uniform_fill(torch.empty_like(un), seed, k) for k in range(S)])
        want = net.plan.cond_ddim_sample(pk, dd, h, un, eta_noise, return_last=return_last)
        got = net.plan.cond_ddim_sample(pk, dd, h, un, return_last=return_last, rng_seed=seed)
        other = net.plan.cond_ddim_sample(pk, dd, h, un, return_last=return_last, rng_seed=seed + 1)
        assert tuple(got[0].shape) == (B, 1 if return_last else S + 1, H, W, 1)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
        assert not torch.equal(other[0], want[0]) and bool(torch.isfinite(other[0]).all()) and bool(torch.isfinite(other[1]).all())
        with pytest.raises(RuntimeError, match="not both"):
            net.plan.cond_ddim_sample(pk, dd, h, un, eta_noise, return_last=return_last, rng_seed=seed)
        # eta = 0: the seed is never read
        d0 = L.cond_ddim_desc(sparams(timesteps=timesteps, eta=0.0, w=0.5), alphas_ext(), 1, True)
        a = net.plan.cond_ddim_sample(pk, d0, h, un, return_last=return_last, rng_seed=seed)
        b = net.plan.cond_ddim_sample(pk, d0, h, un, return_last=return_last, rng_seed=seed + 1)
        c = net.plan.cond_ddim_sample(pk, d0, h, un, return_last=return_last)
        assert torch.equal(a[0], b[0]) and torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])


@pytest.fixture(scope="module")
def ddpm_net(L):
    cfg = fx.CFG_D
    plan = L.DdpmPlan(cfg.in_channels, cfg.out_ch, cfg.ch, cfg.ch_mult, cfg.num_res_blocks, cfg.attn_resolutions, cfg.resolution)
    P = dorc.make_params(cfg, 21)
    return plan, plan.pack({k: v.cuda() for k, v in P.items()}, dorc.timestep_freqs(cfg.ch).cuda())


@pytest.mark.parametrize("return_last", [False, True])
def test_ddim_repaint_sample_rng_equals_the_materialised_draws(L, ddpm_net, return_last):
    plan, packed = ddpm_net
    cfg = fx.CFG_D
    N, skip, eta, R, nth, ntu = fx.DDIM_CASES["quad_eta_r3"]
    h, u, init, _ = fx.ddim_inputs("quad_eta_r3")
    hu = torch.cat([h, u], dim=-1).permute(0, 3, 1, 2).contiguous().cuda()
    init = init.cuda()
    ae = dorc.alphas_ext_of(dorc.betas_of(cfg))
    dd, keep = L.ddim_desc(dorc.DdimParams(timesteps=N, skip_type=skip, eta=eta, n_repeat=R, n_time_h=nth, n_time_u=ntu), ae, 1, 1, True)
    S = len(L.ddim_timesteps(cfg.num_timesteps, N, skip))
    seed = dev_seed(31337)
    eta_noise = torch.stack([L.uniform_fill(torch.empty_like(init), seed, k) for k in range(S)])
    want = plan.ddim_repaint_sample(packed, dd, hu, init, eta_noise, return_last=return_last)
    got = plan.ddim_repaint_sample(packed, dd, hu, init, return_last=return_last, rng_seed=seed)
    other = plan.ddim_repaint_sample(packed, dd, hu, init, return_last=return_last, rng_seed=seed + 1)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert not torch.equal(other[0], want[0]) and bool(torch.isfinite(other[0]).all()) and bool(torch.isfinite(other[1]).all())
    with pytest.raises(RuntimeError, match="not both"):
        plan.ddim_repaint_sample(packed, dd, hu, init, eta_noise, return_last=return_last, rng_seed=seed)
    d0, keep0 = L.ddim_desc(dorc.DdimParams(timesteps=N, skip_type=skip, eta=0.0, n_repeat=R, n_time_h=nth, n_time_u=ntu), ae, 1, 1, True)
    a = plan.ddim_repaint_sample(packed, d0, hu, init, return_last=return_last, rng_seed=seed)
    b = plan.ddim_repaint_sample(packed, d0, hu, init, return_last=return_last, rng_seed=seed + 1)
    c = plan.ddim_repaint_sample(packed, d0, hu, init, return_last=return_last)
    assert torch.equal(a[0], b[0]) and torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])


def _cond_edm_module(golden, dx_cond=False, **sampler):
    """PlCondEdm on the small ADM network with SWE residuals; dx_cond: the dx_enc form."""
    from mcedm_amd.ddim import PlCondEdm
    hp = cond_hparams(**sampler)
    cfg = fx.CFG_C
    if dx_cond:
        import dataclasses
        hp.model.update(dx_cond=True, cat_dx=False, dx_norm="prob", dx_detach=True)
        cfg = dataclasses.replace(fx.CFG_C, dx_channels=1, dx_mode="enc")
    m = PlCondEdm(hp).cuda()
    P = orc.make_params(cfg, int(golden("dxcond.npz" if dx_cond else "cond_edm.npz")["seed"]))
    with torch.no_grad():
        for n, p in m.model.named_parameters():
            p.copy_(P[n])
        for n, p in m.ema_model.ma_model.named_parameters():
            p.copy_(P[n])
    st = fx.STEP_NORM_STATS
    m.normalizer_input.set_stats(torch.tensor(st[0]), torch.tensor(st[1]))
    m.normalizer_target.set_stats(torch.tensor(st[2]), torch.tensor(st[3]))
    m.set_pde_loss_function("swe_per", False)
    m.noise_source = "device"
    return m


@pytest.mark.parametrize("return_last", [False, True])
@pytest.mark.parametrize("dx_cond", [False, True])
def test_guided_heun_sampler_rng_equals_the_materialised_draws(L, golden, dx_cond, return_last):
    """Plan.sample with SWE guidance (mcedm_heun_sample_guided_rng) and with dx_input plus guidance (mcedm_heun_sample_dxcond_rng)."""
    N = 4
    m = _cond_edm_module(golden, dx_cond)
    net = m.ema_model.ma_model
    gd = m.pde_loss.guidance_desc(m.normalizer_input, m.normalizer_target, H, W)
    kw = dict(guidance=gd, dx_input=gd if dx_cond else None, return_last=return_last)
    h, u_noise, _ = fx.cond_sampler_inputs("det")
    h, init = h.permute(0, 3, 1, 2).contiguous().cuda(), u_noise.permute(0, 3, 1, 2).contiguous().cuda()
    seed = dev_seed(2718)
    with torch.no_grad():
        pk = net.packed_weights()
        sd = L.sampler_desc(orc.SamplerParams(timesteps=N, S_churn=15.0), 1.0, 0.002, 80.0)
        steps = torch.stack([L.normal_fill(torch.empty(tuple(init.shape), dtype=torch.float64, device="cuda"), seed, i) for i in range(N)])
        want = net.plan.sample(pk, sd, h, None, init, steps, **kw)
        got = net.plan.sample(pk, sd, h, None, init, None, rng_seed=seed, **kw)
        other = net.plan.sample(pk, sd, h, None, init, None, rng_seed=seed + 1, **kw)
        assert tuple(got.shape) == (B, 1 if return_last else N + 1, H, W, 1)
        assert torch.equal(got, want)
        assert not torch.equal(other, want) and bool(torch.isfinite(other).all())
        with pytest.raises(RuntimeError, match="not both"):
            net.plan.sample(pk, sd, h, None, init, steps, rng_seed=seed, **kw)
        # no churn: the seed is never read
        s0 = L.sampler_desc(orc.SamplerParams(timesteps=N, S_churn=0.0), 1.0, 0.002, 80.0)
        a = net.plan.sample(pk, s0, h, None, init, None, rng_seed=seed, **kw)
        b = net.plan.sample(pk, s0, h, None, init, None, rng_seed=seed + 1, **kw)
        assert torch.equal(a, b) and torch.equal(a, net.plan.sample(pk, s0, h, None, init, None, **kw))


# ---- the four module calls ---------------------------------------------------------------------------------------------
def _same(a, b):
    a, b = (a if isinstance(a, tuple) else (a,)), (b if isinstance(b, tuple) else (b,))
    return all(torch.equal(x, y) for x, y in zip(a, b))


def _finite(a):
    return all(bool(torch.isfinite(x).all()) for x in (a if isinstance(a, tuple) else (a,)))


def _no_noise_tensor(monkeypatch):
    """torch.randn / torch.rand must never be asked for a [N or S, B, C, H, W] tensor."""
    def guard(real, name):
        def fn(*a, **k):
            shape = tuple(a[0]) if len(a) == 1 and isinstance(a[0], (tuple, list, torch.Size)) else a
            assert len(shape) < 5, f"the sampler materialised its per-step noise: torch.{name}{shape}"
            return real(*a, **k)
        return fn
    monkeypatch.setattr(torch, "randn", guard(torch.randn, "randn"))
    monkeypatch.setattr(torch, "rand", guard(torch.rand, "rand"))


def _device_noise_contract(m, call, quiet_call, wrapper, buffer_attr, monkeypatch):
    """call(): one sampling call that draws per-step noise; quiet_call(): the same sampler configured to draw none.  The module
    comes with noise_source "device" (or, PlDdim, without the attribute)."""
    assert getattr(m, "noise_source", "device") == "device"

    def run(seed, fn=call):
        torch.manual_seed(seed)
        return fn()
    with monkeypatch.context() as mp:
        _no_noise_tensor(mp)
        a, b, c = run(3), run(3), run(4)
        assert len(m._graphs) == 1 and isinstance(next(iter(m._graphs.values())), wrapper)
        g = next(iter(m._graphs.values()))
        assert getattr(g, buffer_attr) is None and g.seed is not None and g.seed.dtype == torch.int64
        assert _same(a, b) and not _same(a, c) and _finite(a) and _finite(c)
        mp.setenv("MCEDM_HIP_GRAPH", "0")
        assert _same(a, run(3)), "graph replay and eager launches differ for the same seed"
        mp.delenv("MCEDM_HIP_GRAPH")
        # a call that draws nothing takes nothing from torch's CPU generator (the caller's randn_like draws are on the device)
        torch.manual_seed(11)
        before = torch.get_rng_state()
        q = quiet_call()
        assert torch.equal(torch.get_rng_state(), before) and _finite(q)
        assert any(isinstance(v, wrapper) and v.seed is None and getattr(v, buffer_attr) is None for v in m._graphs.values())
    m.noise_source = "elsewhere"
    with pytest.raises(RuntimeError, match="noise_source must be 'device' or 'torch'"):
        call()


def _cond_inputs():
    return fx.randn("cddim/ddim/h", B, H, W, 1).cuda(), fx.randn("cddim/ddim/u_noise", B, H, W, 1).cuda()


@pytest.mark.parametrize("guided", [False, True])
def test_plcondedm_sample_edm_with_device_noise(L, golden, monkeypatch, guided):
    m = _cond_edm_module(golden, timesteps=4, S_churn=15.0)
    sp, quiet = cond_hparams(timesteps=4, S_churn=15.0).sampler, cond_hparams(timesteps=4, S_churn=0.0).sampler
    h, un = _cond_inputs()
    _device_noise_contract(m, lambda: m.sample_edm(h, un, sp, return_last=True, guide_dx=guided),
                           lambda: m.sample_edm(h, un, quiet, return_last=True, guide_dx=guided), L.GraphedSampler, "step_noise",
                           monkeypatch)


def test_plcondedm_dx_cond_sample_edm_with_device_noise(L, golden, monkeypatch):
    m = _cond_edm_module(golden, dx_cond=True, timesteps=4, S_churn=15.0)
    sp, quiet = cond_hparams(timesteps=4, S_churn=15.0).sampler, cond_hparams(timesteps=4, S_churn=0.0).sampler
    h, un = _cond_inputs()
    _device_noise_contract(m, lambda: m.sample_edm(h, un, sp, return_last=True, guide_dx=True),
                           lambda: m.sample_edm(h, un, quiet, return_last=True, guide_dx=True), L.GraphedSampler, "step_noise",
                           monkeypatch)


def test_plcondddim_sample_edm_with_device_noise(L, golden, monkeypatch):
    m = make_module(golden, timesteps=4, S_churn=15.0, w=0.5)
    m.noise_source = "device"
    sp = m.sparams
    quiet = wrap(dict(sp, S_churn=0.0))
    m.set_test_sampler_params(sp)
    h, un = _cond_inputs()
    _device_noise_contract(m, lambda: m.sample_edm(h, un, sp, return_last=False),
                           lambda: m.sample_edm(h, un, quiet, return_last=False), L.GraphedVpSampler, "step_noise", monkeypatch)


def test_plcondddim_sample_with_device_noise(L, golden, monkeypatch):
    m = make_module(golden, **dict(sparams(timesteps=4, eta=0.5, w=0.5)))
    m.noise_source = "device"
    sp, quiet = m.sparams, sparams(timesteps=4, eta=0.0, w=0.5)
    h, un = _cond_inputs()
    _device_noise_contract(m, lambda: m.sample(h, un, sp, return_last=False), lambda: m.sample(h, un, quiet, return_last=False),
                           L.GraphedCondDdim, "eta_noise", monkeypatch)


def _ddim_sampler(eta, N=4, skip="quad", R=3, nth=8, ntu=0):
    return wrap(dict(name="ddim", type="ddim", timesteps=N, skip_type=skip, eta=eta, n_samples=1, n_repeat=R, n_time_h=nth, n_time_u=ntu,
                     return_last=True, select_by_pde=False, use_gt_pde_select=True, guide_dx=False, w=0.0, plot_scaled=False))


def _plddim(sp):
    from mcedm_amd.ddim import PlDdim
    m = PlDdim(ddpm_hparams(sp)).cuda()
    P = dorc.make_params(fx.CFG_D, 21)
    with torch.no_grad():
        for n, p in m.model.named_parameters():
            p.copy_(P[n])
        for n, p in m.ema_model.ma_model.named_parameters():
            p.copy_(P[n])
    return m


def test_plddim_sample_with_repeat_with_device_noise(L, monkeypatch):
    N, skip, eta, R, nth, ntu = fx.DDIM_CASES["quad_eta_r3"]
    sp, quiet = _ddim_sampler(eta, N, skip, R, nth, ntu), _ddim_sampler(0.0, N, skip, R, nth, ntu)
    m = _plddim(sp)
    assert "noise_source" not in vars(m)                               # absent means "device"
    h, u, _, _ = fx.ddim_inputs("quad_eta_r3")
    h, u = h.cuda(), u.cuda()

    def call(s=sp):
        torch.cuda.manual_seed(5)                                          # the sampler's own randn_like(hu)
        return m.sample_with_repeat(h, u, s, return_last=False)
    _device_noise_contract(m, call, lambda: call(quiet), L.GraphedDdimRepaint, "eta_noise", monkeypatch)


# ---- the two calls that gained graph replay, under "torch" ------------------------------------------------------------------
def test_plddim_sample_with_repeat_graph_replay_equals_eager_under_torch(L, monkeypatch):
    N, skip, eta, R, nth, ntu = fx.DDIM_CASES["quad_eta_r3"]
    sp = _ddim_sampler(eta, N, skip, R, nth, ntu)
    h, u, _, _ = fx.ddim_inputs("quad_eta_r3")
    inputs = [(h.cuda(), u.cuda()), (fx.randn("noise/ddim/h2", *h.shape).cuda(), fx.randn("noise/ddim/u2", *u.shape).cuda())]
    got = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("MCEDM_HIP_GRAPH", mode)
        m = _plddim(sp)
        m.noise_source = "torch"
        res = []
        for k, (hh, uu) in enumerate(inputs):
            torch.manual_seed(100 + k)
            res.append(m.sample_with_repeat(hh, uu, sp, return_last=False))
        if mode == "1":
            g = next(iter(m._graphs.values()))
            assert len(m._graphs) == 1 and isinstance(g, L.GraphedDdimRepaint) and g.seed is None and g.eta_noise is not None
        else:
            assert not m._graphs
        got[mode] = res
    for a, b in zip(got["1"], got["0"]):
        assert _same(a, b) and _finite(a)
    assert not _same(got["1"][0], got["1"][1])


def test_plcondddim_sample_edm_graph_replay_equals_eager_under_torch(L, golden, monkeypatch):
    h, un = _cond_inputs()
    inputs = [(h, un), (fx.randn("noise/vp/h2", B, H, W, 1).cuda(), fx.randn("noise/vp/u2", B, H, W, 1).cuda())]
    got = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("MCEDM_HIP_GRAPH", mode)
        m = make_module(golden, timesteps=4, S_churn=15.0, w=0.5)
        m.noise_source = "torch"
        m.set_test_sampler_params(m.sparams)
        res = []
        for k, (hh, uu) in enumerate(inputs):
            torch.manual_seed(100 + k)
            res.append(m.sample_edm(hh, uu, m.sparams, return_last=False))
        if mode == "1":
            g = next(iter(m._graphs.values()))
            assert len(m._graphs) == 1 and isinstance(g, L.GraphedVpSampler) and g.seed is None and g.step_noise is not None
        else:
            assert not m._graphs
        got[mode] = res
    for a, b in zip(got["1"], got["0"]):
        assert _same(a, b) and _finite(a)
    assert not _same(got["1"][0], got["1"][1])
