"""GPU: PlCondDdim.sample, the DDIM sampler of the single-task conditional DDPM on the ADM U-Net with self-conditioning
(reference models/ddim.py:1452-1530; mcedm_cond_ddim_sample), against the reference's own runs
(tests/golden/cond_ddim_sample.npz, written by tools/make_golden_cond_ddim_sample.py with every random draw injected), its step
kernel against an fp64 restatement, the workspace size, the argument checks, graph replay and the two evaluation loops."""
import numpy as np
import pytest
import torch

from oracle import fixtures as fx
from oracle import mcedm_oracle as orc
from tests._tol import close_per_entry
from tests.test_cond_ddim_sample_cpu import alphas_ext, sparams
from tests.test_hip_cond_ddim import CFG, B, H, W, make_module
from tests.test_hip_eval_steps import _compare, _fill

pytestmark = pytest.mark.gpu

# tag -> (timesteps, skip_type, eta, w): the generator's CASES
CASES = {"uni": (10, "uniform", 0.0, 0.0), "cfg_eta": (10, "uniform", 0.5, 0.5), "quad": (8, "quad", 0.0, 0.0),
         "uneven": (7, "uniform", 0.0, 0.0)}
STEPS = {"uni": 10, "cfg_eta": 10, "quad": 8, "uneven": 8}       # 1000 // 7 = 142 walks 8 timesteps


def inputs():
    return fx.randn("cddim/ddim/h", B, H, W, 1).cuda(), fx.randn("cddim/ddim/u_noise", B, H, W, 1).cuda()


def eta_draw(tag, k):
    """Step k's torch.rand_like(x) of models/ddim.py:1512 as the generator injected it: a tagged uniform in [0, 1)."""
    return torch.from_numpy(((fx.uniform(f"cddim/ddim/{tag}/eta{k}", B, 1, H, W) + 1.0) * 0.5).astype(np.float32))


def ddim_module(golden, **over):
    d = dict(sparams(**over))
    return make_module(golden, **d)


@pytest.mark.parametrize("tag", list(CASES))
def test_sample_golden(golden, monkeypatch, tag):
    """Both trajectories, every slot, at the trajectory bar (rtol 1e-4, atol 1e-5 x max|slot|); return_last is the last slot."""
    g = golden("cond_ddim_sample.npz")
    N, skip, eta, w = CASES[tag]
    m = ddim_module(golden, timesteps=N, skip_type=skip, eta=eta, w=w)
    h, un = inputs()
    S = STEPS[tag]
    draws = torch.stack([eta_draw(tag, k) for k in range(S)]).cuda()
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
    assert tuple(xs_last.shape) == tuple(x0_last.shape) == (B, 1, H, W, 1)
    assert torch.equal(xs[:, 0], un)
    print(f"{tag}: xs worst err / bar {close_per_entry(xs, g[f'{tag}::xs'], what=f'{tag} xs'):.4f}, "
          f"x0_preds {close_per_entry(x0, g[f'{tag}::x0_preds'], what=f'{tag} x0_preds'):.4f}")
    assert torch.equal(xs_last[:, 0], xs[:, -1]) and torch.equal(x0_last[:, 0], x0[:, -1])


def _f32(v):
    return float(np.float32(v))


@pytest.mark.parametrize("stochastic", [False, True])
@pytest.mark.parametrize("guided", [False, True])
@pytest.mark.parametrize("shape", [(3, 1, 32, 32), (1, 1, 5, 7), (2, 2, 6, 6), (2, 3, 5, 7)])
def test_step_kernel_against_fp64(shape, guided, stochastic):
    """ddim_cond_step_kernel against the formulas in fp64.  The shapes take the 16-byte body with 16-byte scatter stores
    (H W % 4 == 0, C == 1), the all-scalar path behind a 3-element tail ((1, 1, 5, 7): 35 elements, nothing aligned), vector
    scatter into cond' with scalar trajectory stores (C == 2) and groups of four that straddle samples ((2, 3, 5, 7): 210).

    Bound: rtol 1e-6 on the result plus the rounding of the fp32 intermediates, which cancellation in xt - et * s1 does not
    shrink with the result.  With u = 2^-24 and mag = |w1 F| + |w Fu| (|F| unguided) every product and sum rounds by at most u of
    its magnitude: et carries 3 u mag, et * s1 4 u s1 mag, the difference u |xt| + 5 u s1 mag, the quotient at most
    (2 u |xt| + 6 u s1 mag) / s0 -- bounded by 8 u (|xt| + s1 mag) / s0.  xt_next adds to sa times that the roundings of its own
    three products and two sums, at most 3 u sa |x0| + 2 u |c1 noise| + 5 u c2 mag -- bounded by 6 u (sa |x0| + |c1 noise| + c2 mag)."""
    from mcedm_amd import lib as L
    Bq, Cq, Hq, Wq = shape
    tag = "x".join(map(str, shape))
    xt, F, Fu = (fx.randn(f"cddim/step/{tag}/{k}", *shape).cuda() for k in ("xt", "F", "Fu"))
    nz = torch.from_numpy(fx.uniform(f"cddim/step/{tag}/nz", *shape).astype(np.float32)).cuda()
    w = 0.5
    a_t, a_n = 0.3, 0.55
    s0, s1, sa = _f32(np.sqrt(np.float32(a_t))), _f32(np.sqrt(np.float32(1 - a_t))), _f32(np.sqrt(np.float32(a_n)))
    c1 = _f32(0.4) if stochastic else 0.0
    c2 = _f32(0.6)
    cc, Cp, T = 2, 2 + Cq + 1, 3                                       # cond' = (2 cond channels, x0, one spare channel)
    cond = fx.randn(f"cddim/step/{tag}/cond", Bq, Cp, Hq, Wq).cuda()
    condp, condu = cond.clone(), (cond * 2).clone()
    xs = torch.full((Bq, T + 1, Hq, Wq, Cq), 7.0, device="cuda")
    x0s = torch.full((Bq, T, Hq, Wq, Cq), 7.0, device="cuda")
    xn = L.op_ddim_cond_step(xt, F, s0, s1, sa, c2, Fu=Fu if guided else None, w=w, noise=nz if stochastic else None, c1=c1,
                             condp=condp, condp_u=condu if guided else None, cond_channels=cc, xs=xs, t_xs=2, x0s=x0s, t_x0=1)
    x64, F64, Fu64, nz64 = (t.double() for t in (xt, F, Fu, nz))
    w1f, wf = _f32(w + 1.0), _f32(w)
    et = w1f * F64 - wf * Fu64 if guided else F64
    mag_et = (w1f * F64).abs() + (wf * Fu64).abs() if guided else F64.abs()
    x0_ref = (x64 - et * s1) / s0
    xn_ref = sa * x0_ref + (c1 * nz64 if stochastic else 0.0) + c2 * et
    u = 2.0 ** -24
    tol_x0 = 8 * u * (x64.abs() + s1 * mag_et) / s0
    tol_xn = sa * tol_x0 + 6 * u * (sa * x0_ref.abs() + (c1 * nz64).abs() + c2 * mag_et)
    x0_got = x0s[:, 1].permute(0, 3, 1, 2).double()
    assert bool(((x0_got - x0_ref).abs() <= 1e-6 * x0_ref.abs() + tol_x0).all()), float((x0_got - x0_ref).abs().max())
    assert bool(((xn.double() - xn_ref).abs() <= 1e-6 * xn_ref.abs() + tol_xn).all()), float((xn.double() - xn_ref).abs().max())
    # where the results go: the trajectory slots and nothing else, the self-conditioning channels and nothing else -- bit for bit
    assert torch.equal(xs[:, 2].permute(0, 3, 1, 2), xn)
    assert bool((xs[:, [0, 1, 3]] == 7.0).all()) and bool((x0s[:, [0, 2]] == 7.0).all())
    assert torch.equal(condp[:, cc:cc + Cq], x0s[:, 1].permute(0, 3, 1, 2))
    assert torch.equal(condp[:, :cc], cond[:, :cc]) and torch.equal(condp[:, cc + Cq:], cond[:, cc + Cq:])
    if guided:
        assert torch.equal(condu[:, cc:cc + Cq], condp[:, cc:cc + Cq])
        assert torch.equal(condu[:, :cc], 2 * cond[:, :cc]) and torch.equal(condu[:, cc + Cq:], 2 * cond[:, cc + Cq:])
    else:
        assert torch.equal(condu, 2 * cond)


class _FixedWorkspace:
    def __init__(self, nbytes):
        self.buf = torch.empty(nbytes, dtype=torch.uint8, device="cuda")

    def get(self, nbytes, device):
        return self.buf


def _plan_call(golden, eta=0.0, w=0.5):
    from mcedm_amd import lib as L
    m = ddim_module(golden, timesteps=4, eta=eta, w=w)
    net = m.ema_model.ma_model
    dd = L.cond_ddim_desc(m.sparams, alphas_ext(), 1, True)
    h, un = inputs()
    return net, dd, h.permute(0, 3, 1, 2).contiguous(), un.permute(0, 3, 1, 2).contiguous()


def test_runs_at_exactly_its_workspace_size(golden):
    """The call succeeds in a buffer of exactly cond_ddim_workspace_bytes and returns MCEDM_ERR_WORKSPACE one byte under."""
    net, dd, h, un = _plan_call(golden)
    need = net.plan.cond_ddim_workspace_bytes(B, H, W)
    with torch.no_grad():
        pk = net.packed_weights()
        xs, x0 = net.plan.cond_ddim_sample(pk, dd, h, un, return_last=False, ws=_FixedWorkspace(need))
        ref = net.plan.cond_ddim_sample(pk, dd, h, un, return_last=False, ws=_FixedWorkspace(need + 4096))
        assert torch.isfinite(xs).all() and torch.equal(xs, ref[0]) and torch.equal(x0, ref[1])
        with pytest.raises(RuntimeError, match=r"\(-3\).*workspace too small"):
            net.plan.cond_ddim_sample(pk, dd, h, un, return_last=False, ws=_FixedWorkspace(need - 1))


def test_rejected_calls_launch_nothing(golden):
    """Every argument check of mcedm_cond_ddim_sample returns its error with the outputs and the workspace untouched (the two
    schedule checks, which the binding's own helpers stop first, are exercised at the C level in test_cond_ddim_sample_cpu.py)."""
    from mcedm_amd import lib as L
    net, dd, h, un = _plan_call(golden)
    plan, ae = net.plan, alphas_ext()
    need = plan.cond_ddim_workspace_bytes(B, H, W)
    ws = _FixedWorkspace(need)
    ws.buf.fill_(0x5A)
    out = (torch.full((B, 5, H, W, 1), 3.0, device="cuda"), torch.full((B, 4, H, W, 1), 3.0, device="cuda"))
    plain = L.Plan(1, 1, 1, CFG.ch, CFG.ch_mult, CFG.num_res_blocks, CFG.attn_resolutions, CFG.resolution)
    uneven = L.Plan(2, 2, 1, CFG.ch, CFG.ch_mult, CFG.num_res_blocks, CFG.attn_resolutions, CFG.resolution)
    dxp = L.Plan(1, 2, 1, CFG.ch, CFG.ch_mult, CFG.num_res_blocks, CFG.attn_resolutions, CFG.resolution, dx_channels=1, dx_mode=L.DX_ENC)
    sp3 = lambda **k: sparams(timesteps=4, **k)
    with torch.no_grad():
        pk = net.packed_weights()
        cases = [
            (plan, L.cond_ddim_desc(sp3(eta=0.5), ae, 1, True), h, None, "eta != 0 needs eta_noise"),
            (plan, L.cond_ddim_desc(sp3(), ae, 3, False), h, None, "cond_channels 3 outside"),
            (plan, L.cond_ddim_desc(sp3(), ae, -1, False), h, None, "cond_channels -1 outside"),
            (plan, dd, None, None, "cond goes with cond_channels"),
            (plan, L.cond_ddim_desc(sp3(), ae, 2, True), torch.cat([h, h], 1).contiguous(), None, "not widened"),
            (plain, dd, h, None, "not widened"),
            (uneven, dd, h, None, "in_channels != out_channels"),
            (dxp, dd, h, None, "dx_cond plans"),
        ]
        import ctypes as C
        lib = L.load()

        def raw(p, d, c, en, nbytes=need):
            """The C entry itself on real buffers: the binding's own shape checks stay out of the way."""
            ptr = lambda t: None if t is None else t.data_ptr()
            rc = lib.mcedm_cond_ddim_sample(p, ptr(pk), d, ptr(c), ptr(un), ptr(en), ptr(out[0]), ptr(out[1]), 0, ptr(ws.buf), nbytes,
                                            B, H, W, torch.cuda.current_stream().cuda_stream)
            return rc, lib.mcedm_last_error().decode()
        for p, d, c, en, msg in cases:
            rc, err = raw(p._h, C.byref(d), c, en)
            assert rc == -1 and msg in err, (msg, rc, err)
        rc, err = raw(plan._h, C.byref(dd), h, None, need - 1)
        assert rc == -3 and "workspace too small" in err, (rc, err)
        for hole in range(7):                          # plan, packed, desc, init_noise, xs_out, x0_out, workspace
            a = [plan._h, pk.data_ptr(), C.byref(dd), un.data_ptr(), out[0].data_ptr(), out[1].data_ptr(), ws.buf.data_ptr()]
            a[hole] = None
            rc = lib.mcedm_cond_ddim_sample(a[0], a[1], a[2], h.data_ptr(), a[3], None, a[4], a[5], 0, a[6], need, B, H, W,
                                            torch.cuda.current_stream().cuda_stream)
            assert rc == -1 and b"null argument" in lib.mcedm_last_error(), hole
    torch.cuda.synchronize()
    assert bool((out[0] == 3.0).all()) and bool((out[1] == 3.0).all()) and bool((ws.buf == 0x5A).all())


def test_graph_replay_equals_the_eager_path(golden, monkeypatch):
    """Two calls with the same shapes and different u_noise: replayed from the captured graph (the default) and run eagerly
    (MCEDM_HIP_GRAPH=0), bit for bit -- with guidance and with the up-front uniform draws of eta != 0 (same seed, same draws)."""
    h, un = inputs()
    noises = [un, fx.randn("cddim/ddim/u_noise2", B, H, W, 1).cuda()]
    got = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("MCEDM_HIP_GRAPH", mode)
        m = ddim_module(golden, timesteps=4, eta=0.5, w=0.5)
        res = []
        for k, nz in enumerate(noises):
            torch.manual_seed(100 + k)
            res.append(m.sample(h, nz, m.sparams, return_last=False))
        assert (len(m._graphs) == 1 and all(v != "eager" for v in m._graphs.values())) if mode == "1" else not m._graphs
        got[mode] = res
    for (xa, x0a), (xb, x0b) in zip(got["1"], got["0"]):
        assert torch.equal(xa, xb) and torch.equal(x0a, x0b) and torch.isfinite(xa).all()
    assert not torch.equal(got["1"][0][0], got["1"][1][0])


def _eval_module(golden, **over):
    import mcedm_amd  # noqa: F401
    from mcedm_amd.ddim import PlCondDdim
    from tests.test_cond_ddim_cpu import ddim_hparams
    hp = ddim_hparams(cond_p=0.8)
    hp.sampler = sparams(timesteps=4, **over)
    m = PlCondDdim(hp).cuda()
    P = orc.make_params(CFG, int(golden("cond_ddim_sample.npz")["seed"]))
    logs = _fill(m, P, fx.STEP_NORM_STATS, "swe_per")
    return m, logs


def _eval_inputs(which, n):
    st = fx.STEP_NORM_STATS
    h = fx.randn(f"cddim/ddim/{which}/h", fx.EVAL_B, H, W, 1) * st[1] + st[0]
    u = fx.randn(f"cddim/ddim/{which}/u", fx.EVAL_B, H, W, 1) * st[3] + st[2]
    return h.cuda(), u.cuda(), fx.randn(f"cddim/ddim/{which}/init", n * fx.EVAL_B, H, W, 1)


def test_validation_step_with_the_ddim_sampler_golden(golden, monkeypatch):
    """models/ddim.py:1169-1172 with sparams.type == 'ddim': validation_step samples with self.sample."""
    g = golden("cond_ddim_sample.npz")
    m, logs = _eval_module(golden)
    h, u, init = _eval_inputs("val", 1)
    monkeypatch.setattr(torch, "randn_like", lambda t, **k: init.to(t.device))
    res = m.validation_step((h, None, None, u), 0)
    monkeypatch.undo()
    assert res.pop("epoch") == 0
    _compare(g, "val", res, logs)


def test_test_step_with_the_ddim_sampler_golden(golden, monkeypatch):
    """models/ddim.py:1239-1242 with sparams.type == 'ddim' and n_samples 2."""
    g = golden("cond_ddim_sample.npz")
    m, logs = _eval_module(golden, n_samples=2)
    m.set_test_sampler_params(m.sparams)
    h, u, init = _eval_inputs("test", 2)
    monkeypatch.setattr(torch, "randn_like", lambda t, **k: init.to(t.device))
    res = m.test_step((h, None, None, u), 0)
    monkeypatch.undo()
    _compare(g, "test", res, logs)
