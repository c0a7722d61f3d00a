"""PlCondDdim with PDE guidance (guide_dx=True; reference models/ddim.py:1499-1503 in ``sample``, :1576-1578 and 1589-1590 in
``sample_edm``) on both networks, against the reference's own guided runs (tests/golden/cond_guided*.npz, tools/make_golden_cond_guided.py),
plus the contracts of the guided C entries: gd NULL is the unguided entry, the seed form is the tensor-fed form, the step kernel
against its formula in fp64, graph replay against eager launches, and test_step with ``guide_dx: True`` in the sampler block."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import fixtures as fx
from oracle import mcedm_oracle as orc
from tests import _cond_guided as G
from tests import _ddpm_cond as D
from tests._tol import close_per_entry
from tests.test_cond_ddim_cpu import ddim_hparams
from tests.test_cond_ddim_sample_cpu import alphas_ext, sparams
from tests.test_hip_cond_ddim import CFG
from tests.test_hip_module import wrap

pytestmark = pytest.mark.gpu
B, H, W = G.B, G.H, G.W


def make_module(golden, net, sp, system="swe_per", noise_source="torch"):
    import mcedm_amd  # noqa: F401
    from mcedm_amd.ddim import PlCondDdim
    st = fx.STEP_NORM_STATS
    if net == "adm":
        hp = ddim_hparams(cond_p=0.8)
        hp.sampler = wrap(dict(sp))
        m = PlCondDdim(hp).cuda()
        P = orc.make_params(CFG, int(golden("cond_ddim.npz")["seed"]))
        with torch.no_grad():
            for mod in (m.model, m.ema_model.ma_model):
                for n, p in mod.named_parameters():
                    p.copy_(P[n])
        m.normalizer_input.set_stats(torch.tensor(st[0]).cuda(), torch.tensor(st[1]).cuda())
        m.normalizer_target.set_stats(torch.tensor(st[2]).cuda(), torch.tensor(st[3]).cuda())
    else:
        m = D.fill(PlCondDdim(wrap(D.hparams_dict(dict(sp)))).cuda(), 1, st)
    m.set_pde_loss_function(system, False)
    m.noise_source = noise_source
    logs = {}
    m.log = lambda name, value, **k: logs.__setitem__(name, torch.as_tensor(value).detach().cpu())
    m.current_epoch = 0
    return m, logs


def inject(monkeypatch, tag):
    """torch.rand / torch.randn hand the samplers' up-front draws (noise_source 'torch') the generator's injected tensors."""
    S = G.STEPS[tag]
    eta = torch.stack([G.eta_draw(tag, k) for k in range(S)]).cuda()
    steps = torch.stack(G.step_draws(tag)).cuda()
    real_rand, real_randn = torch.rand, torch.randn

    def shape_of(a):
        return tuple(a[0]) if len(a) == 1 and isinstance(a[0], (tuple, list, torch.Size)) else tuple(a)
    monkeypatch.setattr(torch, "rand", lambda *a, **k: eta.clone() if shape_of(a) == tuple(eta.shape) else real_rand(*a, **k))
    monkeypatch.setattr(torch, "randn", lambda *a, **k: steps.clone() if shape_of(a) == tuple(steps.shape) and k.get("dtype") == torch.float64
                        else real_randn(*a, **k))


def run(m, tag, guide, return_last=False, un=None):
    h, u0 = G.inputs()
    un = u0 if un is None else un
    sp = wrap(G.sampler_dict(tag, guide_dx=guide))
    if G.CASES[tag][0] == "sample":
        return m.sample(h.cuda(), un.cuda(), sp, return_last=return_last, guide_dx=guide)
    m.set_test_sampler_params(sp)
    return m.sample_edm(h.cuda(), un.cuda(), sp, return_last=return_last, guide_dx=guide), None


# ---- 1. the reference's own guided runs ---------------------------------------------------------------------------------
@pytest.mark.parametrize("net,tag", [(n, t) for n in G.NETS for t in G.cases_of(n)])
def test_guided_golden(golden, monkeypatch, net, tag):
    """Every recorded slot at the trajectory bar (rtol 1e-4, atol 1e-5 x max|slot|); return_last is the last slot bit for bit; the
    unguided call matches the reference's unguided state, and guidance moves the state by more than 10 x the parity error."""
    g = golden(G.GOLDEN[net])
    key, S = f"{net}::{tag}", G.STEPS[tag]
    n = int(g[f"{key}::slots"])
    m, _ = make_module(golden, net, G.sampler_dict(tag), G.CASES[tag][1])
    inject(monkeypatch, tag)
    xs, x0 = run(m, tag, True)
    xs_last, x0_last = run(m, tag, True, return_last=True)
    plain, _ = run(m, tag, False)
    monkeypatch.undo()
    assert tuple(xs.shape) == (B, S + 1, H, W, 1) and tuple(xs_last.shape) == (B, 1, H, W, 1)
    assert torch.isfinite(xs[:, :n + 1]).all()
    err = close_per_entry(xs[:, :n + 1], g[f"{key}::xs"][:, :n + 1], what=f"{key} xs")
    if x0 is not None:
        assert xs.dtype == x0.dtype == torch.float32
        err = max(err, close_per_entry(x0[:, :n], g[f"{key}::x0_preds"][:, :n], what=f"{key} x0_preds"))
        assert torch.equal(x0_last[:, 0], x0[:, -1])
    else:
        assert xs.dtype == torch.float64
    assert torch.equal(xs_last[:, 0], xs[:, -1])
    perr = close_per_entry(plain[:, n:n + 1], g[f"{key}::unguided_last"], what=f"{key} unguided")
    moved = G.bars_apart(xs[:, n].cpu(), plain[:, n].cpu())
    print(f"{key}: {n} steps, parity worst err / bar {err:.4f} (unguided {perr:.4f}), guidance moves slot {n} by {moved:.4g} x bar")
    if tag != "darcy":                        # the Darcy log-probability gradient is exactly 0 on these states in the reference too
        assert moved > 10.0 * max(err, perr)


# ---- 2. / 3. the C entries: gd NULL is the unguided entry; the seed form is the tensor-fed form -------------------------------------
def _raw_guided(plan, stem, pk, sd, gd, cond, init, noise, seed, shapes, dtype, nbytes):
    from mcedm_amd import lib as L
    ptr = lambda t: None if t is None else t.data_ptr()      # noqa: E731
    outs = [torch.full(s, 7.0, dtype=dtype, device="cuda") for s in shapes]
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    rc = getattr(L.load(), L.GUIDED_ENTRIES[stem])(plan._h, pk.data_ptr(), C.byref(sd), None if gd is None else C.byref(gd), ptr(cond),
                                                   ptr(init), ptr(noise), ptr(seed), *[o.data_ptr() for o in outs], 0, ws.data_ptr(),
                                                   ws.numel(), *plan._dims(B, H, W), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, L.load().mcedm_last_error().decode()
    return outs


@pytest.mark.parametrize("kind", ["ddim", "vp"])
@pytest.mark.parametrize("net", G.NETS)
def test_guided_entries_null_description_and_seed_form(golden, net, kind):
    from mcedm_amd import lib as L
    m, _ = make_module(golden, net, G.sampler_dict("ddim"))
    netm = m._net(m.ema_model)
    plan = netm.plan
    h, un = G.inputs()
    cond, init = h.permute(0, 3, 1, 2).contiguous().cuda(), un.permute(0, 3, 1, 2).contiguous().cuda()
    gd = m.pde_loss.guidance_desc(m.normalizer_input, m.normalizer_target, H, W)
    seed = torch.tensor([20240611], dtype=torch.int64, device="cuda")
    if kind == "ddim":
        sd = L.cond_ddim_desc(sparams(timesteps=4, eta=0.5, w=0.5), alphas_ext(), 1, True)
        S = 4
        noise = torch.empty((S, B, 1, H, W), device="cuda")
        for k in range(S):
            L.uniform_fill(noise[k], seed, k)
        call, stem = plan.cond_ddim_sample, f"mcedm_{plan._WHAT}cond_ddim_sample"
        shapes, dtype, query = [(B, S + 1, H, W, 1), (B, S, H, W, 1)], torch.float32, plan.cond_ddim_workspace_bytes
        kw_noise = "eta_noise"
    else:
        # three steps from sigma 5, the first two churn; c_noise: any labels of the schedule table
        sd = L.vp_sampler_desc(3, 1, [5.0, 2.0, 0.5, 0.0], [5.5, 2.2, 0.5], [100.0, 200.0, 300.0, 400.0, 500.0, 600.0], 1.0, 0.5)
        S = 3
        noise = torch.empty((S, B, 1, H, W), dtype=torch.float64, device="cuda")
        for k in range(S):
            L.normal_fill(noise[k], seed, k)
        call, stem = plan.vp_sample, f"mcedm_{plan._WHAT}vp_heun_sample"
        shapes, dtype, query = [(B, S + 1, H, W, 1)], torch.float64, plan.vp_sampler_workspace_bytes
        kw_noise = "step_noise"
    as_list = lambda r: list(r) if isinstance(r, tuple) else [r]      # noqa: E731
    with torch.no_grad():
        pk = netm.packed_weights()
        nbytes = query(B, H, W, guided=True)
        plain_t = as_list(call(pk, sd, cond, init, return_last=False, **{kw_noise: noise}))
        plain_s = as_list(call(pk, sd, cond, init, return_last=False, rng_seed=seed))
        null_t = _raw_guided(plan, stem, pk, sd, None, cond, init, noise, None, shapes, dtype, nbytes)
        null_s = _raw_guided(plan, stem, pk, sd, None, cond, init, None, seed, shapes, dtype, nbytes)
        guided_t = as_list(call(pk, sd, cond, init, return_last=False, guidance=gd, **{kw_noise: noise}))
        guided_s = as_list(call(pk, sd, cond, init, return_last=False, guidance=gd, rng_seed=seed))
    for a, b, c, d, e, f in zip(plain_t, plain_s, null_t, null_s, guided_t, guided_s):
        assert torch.isfinite(a).all() and torch.isfinite(e).all()
        assert torch.equal(c, a) and torch.equal(d, b)                     # gd NULL: the unguided entry, bit for bit
        assert torch.equal(e, f)                                           # with guidance, the seed form is the tensor-fed form
        assert not torch.equal(e[:, 1:], a[:, 1:])                         # and the description is heard


# ---- 4. the step kernel ------------------------------------------------------------------------------------------------
def _f32(v):
    return float(np.float32(v))


@pytest.mark.parametrize("stochastic", [False, True])
@pytest.mark.parametrize("cfg", [False, True])
@pytest.mark.parametrize("shape", [(3, 1, 32, 32), (1, 1, 5, 7), (2, 1, 6, 6)])
def test_guided_step_kernel_against_fp64(shape, cfg, stochastic):
    """ddim_cond_step_kernel with the guidance term against the formulas in fp64.  The shapes take the 16-byte body with 16-byte
    scatter stores ((3, 1, 32, 32)), the all-scalar path behind a 3-element tail ((1, 1, 5, 7): 35 elements, nothing aligned) and a
    second small body ((2, 1, 6, 6)).

    Bound, extending test_step_kernel_against_fp64's (tests/test_hip_cond_ddim_sample.py): rtol 1e-6 on the result plus the
    rounding of the fp32 intermediates.  With u = 2^-24 and mag = |w1 F| + |w Fu| + |gw dx| (|F| + |gw dx| without the blend) the
    blended et carries 3 u mag as before; the new product gw * dx rounds by u |gw dx| <= u mag and the new difference by at most
    u mag: et carries 5 u mag, et * s1 6 u s1 mag, the difference u |xt| + 7 u s1 mag, the quotient at most
    (2 u |xt| + 8 u s1 mag) / s0 -- bounded by 10 u (|xt| + s1 mag) / s0.  xt_next adds to sa times that the roundings of its own
    three products and two sums on top of et's error, at most 3 u sa |x0| + 2 u |c1 noise| + 7 u c2 mag -- bounded by
    8 u (sa |x0| + |c1 noise| + c2 mag).  (Two roundings more than the unguided 8 u and 6 u.)"""
    from mcedm_amd import lib as L
    Bq, Cq, Hq, Wq = shape
    tag = "x".join(map(str, shape))
    xt, F, Fu, dx = (fx.randn(f"cguided/step/{tag}/{k}", *shape).cuda() for k in ("xt", "F", "Fu", "dx"))
    nz = torch.from_numpy(((fx.uniform(f"cguided/step/{tag}/nz", *shape) + 1.0) * 0.5).astype(np.float32)).cuda()
    seed = torch.tensor([77], dtype=torch.int64, device="cuda")
    w, a_t, a_n = 0.5, 0.3, 0.55
    s0, s1, sa = _f32(np.sqrt(np.float32(a_t))), _f32(np.sqrt(np.float32(1 - a_t))), _f32(np.sqrt(np.float32(a_n)))
    gw = _f32(np.float32(G.WEIGHT) * np.float32(s1))                       # fl(5 * s1), as the loop forms it
    c1, c2 = (_f32(0.4) if stochastic else 0.0), _f32(0.6)
    cc, Cp, T = 2, 2 + Cq + 1, 3
    cond = fx.randn(f"cguided/step/{tag}/cond", Bq, Cp, Hq, Wq).cuda()

    def step(dx_arg, gw_arg, rng=False):
        condp, condu = cond.clone(), (cond * 2).clone()
        xs = torch.full((Bq, T + 1, Hq, Wq, Cq), 7.0, device="cuda")
        x0s = torch.full((Bq, T, Hq, Wq, Cq), 7.0, device="cuda")
        noise = dict(rng_seed=seed, draw=3) if rng else dict(noise=nz if stochastic else None)
        xn = L.op_ddim_cond_step(xt, F, s0, s1, sa, c2, Fu=Fu if cfg else None, w=w, c1=c1, condp=condp, condp_u=condu if cfg else None,
                                 cond_channels=cc, xs=xs, t_xs=2, x0s=x0s, t_x0=1, dx=dx_arg, gw=gw_arg, **noise)
        return xn, xs, x0s, condp, condu
    xn, xs, x0s, condp, condu = step(dx, gw)
    x0_ref, xn_ref, mag = G.ddim_step_fp64(xt, F, Fu if cfg else None, nz if stochastic else None, dx, w, gw, s0, s1, sa, c1, c2)
    u = 2.0 ** -24
    tol_x0 = 10 * u * (xt.double().abs() + s1 * mag) / s0
    tol_xn = sa * tol_x0 + 8 * u * (sa * x0_ref.abs() + ((c1 * nz.double()).abs() if stochastic else 0.0) + c2 * mag)
    x0_got = x0s[:, 1].permute(0, 3, 1, 2).double()
    e0, en = (x0_got - x0_ref).abs(), (xn.double() - xn_ref).abs()
    print(f"{tag} cfg {cfg} stochastic {stochastic}: x0 worst err / bound {float((e0 / (1e-6 * x0_ref.abs() + tol_x0)).max()):.3f}, "
          f"xt_next {float((en / (1e-6 * xn_ref.abs() + tol_xn)).max()):.3f}")
    assert bool((e0 <= 1e-6 * x0_ref.abs() + tol_x0).all()), float(e0.max())
    assert bool((en <= 1e-6 * xn_ref.abs() + tol_xn).all()), float(en.max())
    # the guidance term is there: without it x0 sits |gw dx| s1 / s0 away
    away = (x0_got - G.ddim_step_fp64(xt, F, Fu if cfg else None, None, None, w, gw, s0, s1, sa, c1, c2)[0]).abs()
    assert float((away - (gw * dx.double()).abs() * s1 / s0).abs().max()) < 1e-4 and float(away.max()) > 0.1
    # where the results go: the trajectory slots and nothing else, the self-conditioning channels and nothing else -- bit for bit
    assert torch.equal(xs[:, 2].permute(0, 3, 1, 2), xn)
    assert bool((xs[:, [0, 1, 3]] == 7.0).all()) and bool((x0s[:, [0, 2]] == 7.0).all())
    assert torch.equal(condp[:, cc:cc + Cq], x0s[:, 1].permute(0, 3, 1, 2))
    assert torch.equal(condp[:, :cc], cond[:, :cc]) and torch.equal(condp[:, cc + Cq:], cond[:, cc + Cq:])
    assert torch.equal(condu[:, cc:cc + Cq], condp[:, cc:cc + Cq]) if cfg else torch.equal(condu, 2 * cond)
    # dx NULL through the guided entry is mcedm_op_ddim_cond_step[_rng], trajectory slots and self-conditioning channels included
    for rng in ([False, True] if stochastic else [False]):
        got = step(None, 0.0, rng)
        noise = dict(rng_seed=seed, draw=3) if rng else dict(noise=nz if stochastic else None)
        condp2, condu2 = cond.clone(), (cond * 2).clone()
        xs2, x0s2 = torch.full_like(xs, 7.0), torch.full_like(x0s, 7.0)
        ref = L.op_ddim_cond_step(xt, F, s0, s1, sa, c2, Fu=Fu if cfg else None, w=w, c1=c1, condp=condp2, condp_u=condu2 if cfg else None,
                                  cond_channels=cc, xs=xs2, t_xs=2, x0s=x0s2, t_x0=1, **noise)
        for a, b in zip(got, (ref, xs2, x0s2, condp2, condu2)):
            assert torch.equal(a, b)
    # with guidance too, the value of an element does not depend on which form drew its noise
    if stochastic:
        drawn = L.uniform_fill(torch.empty_like(xt), seed, 3)
        a = L.op_ddim_cond_step(xt, F, s0, s1, sa, c2, Fu=Fu if cfg else None, w=w, c1=c1, noise=drawn, dx=dx, gw=gw)
        b = L.op_ddim_cond_step(xt, F, s0, s1, sa, c2, Fu=Fu if cfg else None, w=w, c1=c1, rng_seed=seed, draw=3, dx=dx, gw=gw)
        assert torch.equal(a, b)


# ---- 5. graph replay ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["ddim_cfg_eta", "vp_churn_cfg"])
@pytest.mark.parametrize("net", G.NETS)
def test_guided_graph_replay_equals_the_eager_path(golden, monkeypatch, net, tag):
    """Two guided calls with different u_noise, replayed from the captured graph (the default) and launched eagerly
    (MCEDM_HIP_GRAPH=0): bit for bit, device-side draws from the same seeds.  A changed guidance description keys a new capture."""
    noises = [G.inputs()[1], fx.randn("cguided/u_noise2", B, H, W, 1)]
    got = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("MCEDM_HIP_GRAPH", mode)
        m, _ = make_module(golden, net, G.sampler_dict(tag), noise_source="device")
        res = []
        for k, nz in enumerate(noises):
            torch.manual_seed(100 + k)
            res.append(run(m, tag, True, un=nz)[0])
        assert (len(m._graphs) == 1 and all(v != "eager" for v in m._graphs.values())) if mode == "1" else not m._graphs
        got[mode] = res
        if mode == "1":
            st = fx.STEP_NORM_STATS                                        # another residual description: another capture
            m.normalizer_target.set_stats(torch.tensor(st[2]).cuda(), torch.tensor(st[3] * 2.0).cuda())
            torch.manual_seed(100)
            other = run(m, tag, True, un=noises[0])[0]
            assert len(m._graphs) == 2 and all(v != "eager" for v in m._graphs.values())
            assert not torch.equal(other, res[0])
    for a, b in zip(got["1"], got["0"]):
        assert torch.equal(a, b) and torch.isfinite(a).all()
    assert not torch.equal(got["1"][0], got["1"][1])


# ---- 6. the evaluation loop ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("net", G.NETS)
def test_test_step_with_guide_dx_in_the_sampler_block(golden, monkeypatch, net):
    """``guide_dx: True`` in the sampler block (every file under the reference's configs/diff_sampler/ carries the switch) reaches the
    samplers through test_step (models/ddim.py:1239-1242): finite metrics, and a trajectory that differs from guide_dx False."""
    st = fx.STEP_NORM_STATS
    hh = (fx.randn("cguided/test/h", fx.EVAL_B, H, W, 1) * 0.3 * st[1] + st[0]).cuda()
    uu = (fx.randn("cguided/test/u", fx.EVAL_B, H, W, 1) * st[3] + st[2]).cuda()
    init = fx.randn("cguided/test/init", 2 * fx.EVAL_B, H, W, 1)
    out = {}
    for guide in (True, False):
        sp = G.sampler_dict("ddim", guide_dx=guide, n_samples=2)
        m, logs = make_module(golden, net, sp)
        m.set_test_sampler_params(wrap(sp))
        monkeypatch.setattr(torch, "randn_like", lambda t, **k: init.to(t.device))
        res = m.test_step((hh, None, None, uu), 0)
        monkeypatch.undo()
        assert logs and all(bool(torch.isfinite(v).all()) for v in logs.values()), logs
        assert all(bool(torch.isfinite(torch.as_tensor(v)).all()) for v in res.values())
        out[guide] = res["traj"]
    assert out[True].shape == out[False].shape and not torch.equal(out[True], out[False])
