"""GPU: one timestep (noise level) per sample on the DDPM U-Net -- the batched timestep kernel, the bias row per sample of the
tiled, input-resident and Winograd convolutions, mcedm_ddpm_forward_t on every architecture of tests/_ddpm_arch.py against the
reference's outputs (tests/golden/ddpm_pert.npz) and the fp64 oracle, bit equality with the one-timestep entries, batch
independence, mcedm_ddpm_edm_denoise_t against the fp64 formula, and graph capture with t rewritten in place.  The bar is the
project's: rtol 1e-4, atol 1e-5 max|ref| (tests/_ddpm_arch.bar_ratio <= 1)."""
import functools

import pytest
import torch
import torch.nn.functional as F

from oracle import fixtures as fx
from tests import _ddpm_arch as A
from tests import _ddpm_pert as T
from tests.test_hip_ddpm_arch import build, net

pytestmark = pytest.mark.gpu
B = A.B


def dev(v):
    return None if v is None else v.cuda()


def call_t(tag, plan, packed, ts, ws=None, inputs=None, out=None):
    """forward_t at the timesteps ts (one per sample), x_self_cond and cond given where the network takes them."""
    cfg = A.ALL[tag]
    x, xsc, cond = (dev(v) for v in (inputs or A.inputs(tag)))
    t = ts if torch.is_tensor(ts) else torch.tensor(ts, dtype=torch.float32).cuda()
    if cfg.cat_cond:
        return plan.forward_t(packed, x, t, cond=cond, ws=ws, out=out)
    cmap = plan.cond_map(packed, cond) if cfg.cond_channels else None
    return plan.forward_t(packed, x, t, x_self_cond=xsc, cond_map=cmap, ws=ws, out=out)


def call_scalar(tag, plan, packed, t, inputs=None):
    """the one-timestep entry of the plan (forward / forward_cond / forward_cat) on the same inputs"""
    cfg = A.ALL[tag]
    x, xsc, cond = (dev(v) for v in (inputs or A.inputs(tag)))
    if cfg.cat_cond:
        return plan.forward_cat(packed, x, t, cond=cond)
    if cfg.cond_channels:
        return plan.forward_cond(packed, x, t, cond_map=plan.cond_map(packed, cond), x_self_cond=xsc)
    return plan.forward(packed, x, t, x_self_cond=xsc)


@functools.lru_cache(maxsize=None)
def reference64(tag):
    P64 = A.params(tag, torch.float64)
    return {T.key(tag, ts): T.oracle_forward(tag, P64, ts) for ts in T.T_PAIRS}


def inputs5(tag):
    """five samples of the row's inputs (the helper's own are B = 2)"""
    c = A.ALL[tag]
    R = c.resolution
    x = fx.randn(f"ddpmp/{tag}/x5", 5, c.in_channels, R, R)
    xsc = fx.randn(f"ddpmp/{tag}/xsc5", 5, c.in_channels, R, R) if c.self_cond else None
    cond = fx.randn(f"ddpmp/{tag}/cond5", 5, c.cond_channels, R, R) if c.cond_channels else None
    return x, xsc, cond


# ---- 1. the rows of a batch of timesteps -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["narrow", "one", "rows3"])
def test_temb_rows_against_the_formula_and_the_single_timestep_call(tag):
    """ch = 32, ch = 64 and the 2816 rows of the capped grid, at both ends of the DDPM range, an early and a late timestep and an
    EDM label: against the formula in fp64 (on the fp32 products t * freq) at the bar, and row set b == the B = 1 call at t_b."""
    L, plan, packed = net(tag)
    t = torch.tensor(T.T_ROWS, dtype=torch.float32).cuda()
    got = plan.temb_rows(packed, t)
    want = T.temb_rows64(tag, A.params(tag, torch.float64), T.T_ROWS)
    assert tuple(got.shape) == tuple(want.shape) == (len(T.T_ROWS), plan.temb_row_count)
    r = A.bar_ratio(got, want)
    print(f"{tag}: {plan.temb_row_count} rows, worst err / bar {r:.4f}")
    assert r <= 1.0, (tag, r)
    for b in range(len(T.T_ROWS)):
        alone = plan.temb_rows(packed, t[b:b + 1].contiguous())
        assert torch.equal(alone[0], got[b]), (tag, b)
    assert not torch.equal(got[1], got[2])


# ---- 2. a bias row per sample in the convolutions, kernel level ------------------------------------------------------------------
def conv_case(name, Cin, Cout, H, W):
    g = lambda what, *s: fx.randn(f"ddpmp/conv/{name}/{what}", *s)
    x = g("x", 3, Cin, H, W)
    w = g("w", Cout, Cin, 3, 3) / (3.0 * Cin ** 0.5)
    bias = g("b", 3, Cout)                                   # three different rows
    return x, w, bias


def conv64(x, w, bias):
    return F.conv2d(x.double(), w.double(), padding=1) + bias.double()[:, :, None, None]


TILED = [("s64", 64, 64, 8, 8), ("p32", 32, 32, 16, 16), ("m128", 128, 64, 32, 32)]


@pytest.mark.parametrize("resident", [1, 0])
@pytest.mark.parametrize("name,Cin,Cout,H,W", TILED)
def test_conv_bias_per_sample_tiled_and_resident(name, Cin, Cout, H, W, resident):
    """B = 3 with three bias rows == three single-sample calls of mcedm_op_conv with that sample's row, bit for bit, on the
    input-resident kernels (resident = 1) and on the tiled ones (0); 32 -> 32 is a partial channel tile of either."""
    import mcedm_amd  # noqa: F401
    from mcedm_amd import lib as L
    x, w, bias = conv_case(name, Cin, Cout, H, W)
    xd = x.cuda()
    packs = [L.op_pack_conv(w.cuda(), bias[b].cuda()) for b in range(3)]
    wpk, pitch = packs[0][0], packs[0][1].numel()
    table = torch.stack([p[1] for p in packs]).contiguous()
    L.set_conv_resident(resident)
    try:
        L.prof_enable(True)
        got = L.op_conv(xd, None, wpk, table, Cout, 3, coef_batch=0, bias_batch=pitch)
        torch.cuda.synchronize()
        names = [r["name"] for r in L.prof_report()]
        L.prof_enable(False)
        # (a 32-channel conv at 16 x 16 has no input-resident form: the tiled kernel's 32-channel tile serves it either way)
        assert any(n.startswith("conv_resident") for n in names) == (bool(resident) and name != "p32"), names
        for b in range(3):
            alone = L.op_conv(xd[b:b + 1].contiguous(), None, wpk, packs[b][1], Cout, 3, coef_batch=0)
            assert torch.equal(alone[0], got[b]), (name, resident, b, float((alone[0] - got[b]).abs().max()))
    finally:
        L.prof_enable(False)
        L.set_conv_resident(-1)
    if name == "m128":
        r = A.bar_ratio(got, conv64(x, w, bias))
        print(f"{name} resident={resident}: worst err / bar {r:.4f} vs the fp64 convolution")
        assert r <= 1.0, r


@pytest.mark.parametrize("C", [64, 128])
@pytest.mark.parametrize("H,W", [(8, 16), (32, 32)])
def test_conv_bias_per_sample_winograd(C, H, W):
    """The Winograd kernels (64 and 128 output channels per workgroup; one tile and many) in the form the network's conv1 launches,
    swish of the transformed input: outputs and the fused GroupNorm records of B = 3 with three bias rows == three single-sample
    calls, bit for bit."""
    import mcedm_amd  # noqa: F401
    from mcedm_amd import lib as L
    x, w, bias = conv_case(f"wino{C}_{H}", C, C, H, W)
    xd, bd = x.cuda(), bias.cuda().contiguous()
    wino = L.op_pack_conv_wino(w.cuda())
    kw = dict(coef=torch.tensor([0.0, 1.0, 0.0, 0.0]).repeat(C, 1).cuda(), coef_batch=0, act=1, want_sums=True)      # identity rows, swish
    L.prof_enable(True)
    try:
        got, sums = L.op_conv_wino(xd, None, wino, bd, C, bias_batch=C, **kw)
        torch.cuda.synchronize()
        assert [r["name"] for r in L.prof_report()] == [f"conv_wino_kernel<WinoCfg<{C // 32}>, false, true, WinoBiasRows>"]
    finally:
        L.prof_enable(False)
    per = (H // 8) * (W // 16) * (C // 4) * 2               # one (sum, M2) per 8 x 16 tile and 4-channel block of a sample
    assert bool((sums[:3 * per] != 0).any()) and not bool(sums[3 * per:].any())
    for b in range(3):
        alone, s1 = L.op_conv_wino(xd[b:b + 1].contiguous(), None, wino, bd[b].contiguous(), C, **kw)
        assert torch.equal(alone[0], got[b]), (C, H, W, b, float((alone[0] - got[b]).abs().max()))
        assert torch.equal(s1[:per], sums[b * per:(b + 1) * per]), (C, H, W, b)
    assert not torch.equal(sums[:per], sums[per:2 * per])
    if (H, W) == (32, 32):
        xs = x.double()
        r = A.bar_ratio(got, conv64(xs * torch.sigmoid(xs), w, bias))
        print(f"winograd {C} at {H} x {W}: worst err / bar {r:.4f} vs the fp64 convolution")
        assert r <= 1.0, r


def test_conv_launchers_without_it_refuse_a_bias_row_per_sample():
    """Cout = 2 (the small-Cout kernel's shape), the stride-2 conv and a 1 x 1 conv: an error, never a result without the rows."""
    import mcedm_amd  # noqa: F401
    from mcedm_amd import lib as L
    g = lambda what, *s: fx.randn(f"ddpmp/refuse/{what}", *s).cuda()
    for what, Cout, k, rs, H in (("Cout 2", 2, 3, L.RS_NONE, 64), ("stride 2", 64, 3, L.RS_S2, 32), ("1 x 1", 64, 1, L.RS_NONE, 16)):
        w = g(f"w{Cout}{k}", Cout, 64, k, k)
        wpk, bpk = L.op_pack_conv(w, g(f"b{Cout}", Cout))
        table = bpk.repeat(3, 1).contiguous()
        with pytest.raises(RuntimeError, match="bias row per sample"):
            L.op_conv(g(f"x{H}", 3, 64, H, H), None, wpk, table, Cout, k, coef_batch=0, resample=rs, bias_batch=bpk.numel())


# ---- 3. the network against the reference and the fp64 oracle --------------------------------------------------------------------
def held(got, key, g, tag, what=""):
    rg, r64 = A.bar_ratio(got, g[key]), A.bar_ratio(got, reference64(tag)[key])
    print(f"{key}{what}: worst err / bar {rg:.4f} vs the reference's run, {r64:.4f} vs the fp64 oracle")
    assert got.dtype == torch.float32 and bool(torch.isfinite(got).all())
    assert rg <= 1.0 and r64 <= 1.0, (key, what, rg, r64)


@pytest.mark.parametrize("tag", list(A.ALL))
def test_forward_t_golden_and_fp64(golden, tag):
    g = golden("ddpm_pert.npz")
    L, plan, packed = net(tag)
    for ts in T.T_PAIRS:
        held(call_t(tag, plan, packed, ts), T.key(tag, ts), g, tag)


@pytest.mark.parametrize("which", ["conv_wino", "conv_resident"])
@pytest.mark.parametrize("tag", A.SWITCHED)
def test_forward_t_with_a_kernel_family_switched_off(golden, tag, which):
    g = golden("ddpm_pert.npz")
    L, plan, packed = build(tag, **{which: 0})
    for ts in T.T_PAIRS:
        held(call_t(tag, plan, packed, ts), T.key(tag, ts), g, tag, what=f" [{which} = 0]")


# ---- 4. the same bits as the one-timestep entries ----------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", list(A.ALL))
def test_equal_timesteps_give_the_bits_of_the_scalar_entry(tag):
    """every t[b] = 937: forward_t == forward / forward_cond / forward_cat at 937; a second call on the same workspace == the first"""
    L, plan, packed = net(tag)
    ws = L.Workspace()
    first = call_t(tag, plan, packed, (937.0, 937.0), ws=ws).clone()
    want = call_scalar(tag, plan, packed, 937.0)
    assert torch.equal(first, want), (tag, float((first - want).abs().max()))
    again = call_t(tag, plan, packed, (937.0, 937.0), ws=ws)
    assert torch.equal(first, again), tag
    assert ws.buf.numel() == plan.workspace_bytes_t(B)      # it ran in exactly what the query says


@pytest.mark.parametrize("tag", ["one", "wide0", "head_narrow3"])
def test_a_sample_does_not_depend_on_the_rest_of_the_batch(tag):
    """sample k of a B = 5 call at five different timesteps == the B = 1 call of the one-timestep entry at t_k, bit for bit"""
    L, plan, packed = net(tag)
    inp = inputs5(tag)
    got = call_t(tag, plan, packed, T.T_FIVE, inputs=inp)
    for k, t in enumerate(T.T_FIVE):
        one = tuple(None if v is None else v[k:k + 1].contiguous() for v in inp)
        alone = call_scalar(tag, plan, packed, t, inputs=one)
        assert torch.equal(alone[0], got[k]), (tag, k, float((alone[0] - got[k]).abs().max()))
    assert not torch.equal(got[0], got[1])


# ---- 5. EDM preconditioning with a noise level per sample --------------------------------------------------------------------------
@pytest.mark.parametrize("use_cond", [True, False])
@pytest.mark.parametrize("tag", list(A.CATS))
def test_edm_denoise_t_against_the_formula_in_fp64(tag, use_cond):
    L, plan, packed = net(tag)
    x = T.edm_input(tag, T.SIGMAS).cuda().contiguous()
    cond = A.inputs(tag)[2].cuda() if use_cond else None
    sigma = torch.tensor(T.SIGMAS, dtype=torch.float32).cuda()
    ws = L.Workspace()
    D, Fx = plan.edm_denoise_t(packed, x, sigma, cond=cond, sigma_data=T.SIGMA_DATA, want_F=True, ws=ws)
    D64, F64 = T.edm_precond64(tag, A.params(tag, torch.float64), T.SIGMAS, use_cond)
    rD, rF = A.bar_ratio(D, D64), A.bar_ratio(Fx, F64)
    print(f"{tag} cond={use_cond}: worst err / bar D {rD:.4f}, F {rF:.4f}")
    assert rD <= 1.0 and rF <= 1.0, (tag, use_cond, rD, rF)
    assert ws.buf.numel() == plan.workspace_bytes_t(B)
    # without F_out the same D
    assert torch.equal(plan.edm_denoise_t(packed, x, sigma, cond=cond, sigma_data=T.SIGMA_DATA), D)


@pytest.mark.parametrize("tag", list(A.CATS))
def test_edm_denoise_t_at_equal_sigmas_agrees_with_the_scalar_entry(tag):
    """At the bar, not bit for bit: c_noise = ln(sigma) / 4 comes from the device's logf here and from torch's on the host there."""
    L, plan, packed = net(tag)
    sg = 3.0
    x = T.edm_input(tag, (sg, sg)).cuda().contiguous()
    cond = A.inputs(tag)[2].cuda()
    D = plan.edm_denoise_t(packed, x, torch.full((B,), sg).cuda(), cond=cond, sigma_data=T.SIGMA_DATA)
    c_noise = float(torch.tensor(sg, dtype=torch.float32).log() / 4)
    want = plan.edm_denoise(packed, x, sg, c_noise, cond=cond, sigma_data=T.SIGMA_DATA)
    r = A.bar_ratio(D, want.cpu())
    print(f"{tag}: worst err / bar {r:.4f} vs mcedm_ddpm_edm_denoise")
    assert r <= 1.0, (tag, r)


# ---- 7. graph capture: t is read on the device -----------------------------------------------------------------------------------
def test_forward_t_captured_and_replayed_with_t_rewritten_in_place():
    tag = "nrb2"
    L, plan, packed = net(tag)
    device = torch.device("cuda", torch.cuda.current_device())
    x, xsc, _ = (dev(v) for v in A.inputs(tag))
    t = torch.tensor(T.T_PAIRS[0], dtype=torch.float32).cuda()
    out = torch.empty((B, A.ALL[tag].out_ch, x.shape[2], x.shape[3]), dtype=torch.float32, device=device)
    ws = L._PinnedWorkspace(None, plan.workspace_bytes_t(B), device)
    graph = L._capture(lambda: plan.forward_t(packed, x, t, x_self_cond=xsc, ws=ws, out=out), device)
    graph.replay()
    torch.cuda.synchronize()
    first = out.clone()
    assert torch.equal(first, call_t(tag, plan, packed, T.T_PAIRS[0]))
    t.copy_(torch.tensor(T.T_PAIRS[1], dtype=torch.float32))          # in place: the graph reads the same address
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, call_t(tag, plan, packed, T.T_PAIRS[1]))
    assert not torch.equal(out, first)


# ---- 6. the three modules: forward and training_step without gradients ------------------------------------------------------------
def step_module(kind):
    import mcedm_amd  # noqa: F401
    from mcedm_amd.ddim import PlCondDdim, PlCondEdm, PlDdim
    from tests.test_hip_module import wrap
    cls = {"ddim": PlDdim, "cond": PlCondDdim, "edm": PlCondEdm}[kind]
    m = T.step_fill(cls(wrap(T.step_hparams(kind))).cuda(), kind)
    m.logged = {}
    m.log = lambda name, value, **k: m.logged.__setitem__(name, value)
    return m


def draws_patched(mp, kind, rands):
    """torch's generator answered as tools/make_golden_ddpm_pert.py answered the reference's (tests/test_hip_cond_ddim.py:47-56)"""
    noise, t_half, rnd = T.step_draws(kind)
    queue = list(rands)
    mp.setattr(torch, "randn_like", lambda t, **k: noise.to(t.device))
    mp.setattr(torch, "randn", lambda *a, **k: rnd.clone())
    mp.setattr(torch, "randint", lambda *a, **k: t_half.clone())
    mp.setattr(torch, "rand", lambda *a, **k: torch.tensor([queue.pop(0)]))
    return queue


CASES = [(kind, case) for kind in T.STEP_CASES for case in T.STEP_CASES[kind]]


@pytest.mark.parametrize("kind,case", CASES)
def test_module_forward_and_training_step_golden(golden, monkeypatch, kind, case):
    """(output, x0_t) at the bar; the loss against the stored fp64 value within the stored bound (rtol 1e-5: the reference's own
    fp32 loss lies within a quarter of that in every case); training_step twice gives equal bits; the network's calls run in
    exactly workspace_bytes_t."""
    g = golden("ddpm_pert_steps.npz")
    m = step_module(kind)
    rands = T.STEP_CASES[kind][case]
    x, cond = (dev(v) for v in T.step_state(kind))
    noise, _, rnd = T.step_draws(kind)
    h, u = (v.cuda() for v in T.step_batch())
    level = (rnd * m.P_std + m.P_mean).exp().cuda() if kind == "edm" else T.step_t().cuda()
    key = f"{kind}::{case}"
    with torch.no_grad():
        with monkeypatch.context() as mp:
            queue = draws_patched(mp, kind, rands)
            out, x0 = m.forward(x, level, noise.cuda(), cond=cond)
            assert not queue
        ro, rx = A.bar_ratio(out, g[f"{key}::output"]), A.bar_ratio(x0, g[f"{key}::x0_t"])
        losses = []
        for _ in range(2):
            with monkeypatch.context() as mp:
                queue = draws_patched(mp, kind, rands)
                losses.append(m.training_step((h, None, None, u), 0))
                assert not queue
    loss64, rtol = float(g[f"{key}::loss64"]), float(g[f"{key}::loss_bar"])
    rel = abs(float(losses[0].double()) - loss64) / abs(loss64)
    print(f"{key}: output err / bar {ro:.4f}, x0_t {rx:.4f}; loss {float(losses[0]):.9g} vs fp64 {loss64:.12g}: rel {rel:.2e} (bound {rtol:.1e})")
    assert ro <= 1.0 and rx <= 1.0, (key, ro, rx)
    assert rel <= rtol, (key, rel, rtol)
    assert losses[0].dim() == 0 and torch.equal(losses[0], losses[1])
    assert torch.equal(m.logged["train_loss"], losses[1])
    assert m.model._ws.buf.numel() == m.model.plan.workspace_bytes_t(T.SB)


@pytest.mark.parametrize("kind", list(T.STEP_CASES))
def test_modules_refuse_with_gradients_enabled(kind):
    m = step_module(kind)
    assert torch.is_grad_enabled()
    for call in (lambda: m.training_step((None, None, None, None), 0), lambda: m.forward(None, None, None)):
        with pytest.raises(NotImplementedError, match="no backward"):
            call()
    if kind == "edm":
        with pytest.raises(NotImplementedError, match="one noise level for the whole batch"):
            m.model_precond(torch.zeros(3, 1, T.SR, T.SR).cuda(), torch.tensor([1.0, 1.0, 2.0]))
        with torch.no_grad(), pytest.raises(NotImplementedError, match="one noise level for the whole batch"):      # guidance
            m.get_denoised(m.model, torch.zeros(3, 1, T.SR, T.SR).cuda(), torch.tensor([1.0, 1.0, 2.0]), w=0.5)


def test_model_forward_routes_by_the_length_of_t():
    """Model.forward: t with B entries is the per-sample entry (== the plan's forward_t), one entry the scalar one, else ValueError"""
    m = step_module("ddim")
    net = m.model
    x = T.step_state("ddim")[0].cuda()
    t = T.step_t().float().cuda()
    with torch.no_grad():
        got = net(x, t)
        assert torch.equal(got, net.plan.forward_t(net.packed_weights(), x, t))
        assert torch.equal(net(x, t[:1])[0], got[0]) and not torch.equal(net(x, t[:1])[1], got[1])
        with pytest.raises(ValueError):
            net(x, t[:3])
