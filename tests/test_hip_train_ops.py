"""GPU: the kernels that close a training step (csrc/edm.hip: noise inputs, EDM and epsilon losses, squared gradient norm with its
fixed-order grid reduction, clip + Adam + EMA) and optim.FusedAdamEma on top of them, against the fp64 references of
tests/_train_ops.py, beyond the first step from zero moments and at the sizes where the grids are capped.

Bounds.  Adam / EMA: FACTOR (4) x e32, where e32 is what torch's own fp32 Adam loses against fp64 on the same inputs (the
yardstick of tests/_train_ops.py, computed here on the CPU, never taken from the kernel).  Everything else: analytic, in units of
U = 2^-24 (one fp32 rounding), relative to the operands of the expression; derivations stand at the assertions.  Each test
prints the ratio error / bound it measured."""
import pytest
import torch

from tests import _train_ops as T

pytestmark = pytest.mark.gpu
U = T.U


@pytest.fixture(scope="module")
def lib():
    import mcedm_amd  # noqa: F401
    from mcedm_amd import lib as L
    assert torch.cuda.is_available()
    L.load()
    return L


def dev(t):
    return None if t is None else t.detach().contiguous().cuda()


def stream():
    return torch.cuda.current_stream().cuda_stream


def ratio(got, ref, lim):
    """max |got - ref| / lim; ``lim`` a number or a tensor of elementwise bounds (0 where the values must be equal)."""
    err = (got.detach().cpu().double() - ref.double()).abs()
    if not torch.is_tensor(lim):
        return float(err.max()) / lim
    assert bool((err[lim == 0] == 0).all())
    return float((err[lim > 0] / lim[lim > 0]).max()) if bool((lim > 0).any()) else 0.0


def fresh_scratch(L):
    """A reduction scratch area whose partial-sum slots hold a huge finite double: a sum over a slot nobody wrote shows."""
    return torch.full((L.REDUCE_SCRATCH_BYTES,), 0x7F, dtype=torch.uint8, device="cuda")


# ------------------------------------------------------------------------------------------------ clip + Adam + EMA
def device_run(L, row, p0, ema0, grads, m0=None, v0=None, step0=0, lr_at=None, sq_list=None, with_ema=True):
    """One lib.sqnorm + lib.adam_ema_step pair per gradient on buffers that stay on the device.  ``sq_list``: squared norms to
    feed in place of the device's own.  Returns (Run, the squared norms used)."""
    p = dev(p0)
    m = torch.zeros_like(p) if m0 is None else dev(m0)
    v = torch.zeros_like(p) if v0 is None else dev(v0)
    ema = dev(ema0) if (row.ema_beta is not None and with_ema) else None
    clip = row.max_norm is not None
    sq = torch.full((1,), float("nan"), dtype=torch.float64, device="cuda")
    scratch = fresh_scratch(L)
    ps, sqs = [], []
    for k, g in enumerate(grads):
        gd = dev(g)
        if clip:
            if sq_list is None:
                L.sqnorm(gd, sq, scratch=scratch)
            else:
                sq.copy_(sq_list[k])
            sqs.append(sq.clone())
        L.adam_ema_step(p, gd, m, v, ema, step0 + k + 1, lr=row.lr if lr_at is None else lr_at(k), beta1=row.b1, beta2=row.b2,
                        eps=row.eps, weight_decay=row.wd, sqnorm_t=sq if clip else None, max_norm=row.max_norm if clip else 1.0,
                        grad_scale=row.grad_scale, ema_beta=0.999 if row.ema_beta is None else row.ema_beta)
        ps.append(p.clone())
    torch.cuda.synchronize()
    return T.Run([t.cpu() for t in ps], m.cpu(), v.cpu(), None if ema is None else ema.cpu()), sqs


def hold_to_yardstick(got, y, what):
    """Every tensor of the run within FACTOR x e32 of fp64; returns the ratios error / e32."""
    r = {"p": max(ratio(g, r_, e) for g, r_, e in zip(got.p_steps, y.ref.p_steps, y.e32_p)),
         "m": ratio(got.m, y.ref.m, y.e32_m), "v": ratio(got.v, y.ref.v, y.e32_v)}
    if y.ref.ema is not None:
        r["ema"] = ratio(got.ema, y.ref.ema, y.e32_ema)
    print(f"{what}: kernel error / e32 " + ", ".join(f"{k} {x:.2f}" for k, x in r.items())
          + f" (e32 p {y.e32_p[-1]:.2e}, movement {y.movement:.2e})")
    for k, x in r.items():
        assert x <= T.FACTOR, f"{what}: {k} is {x:.2f} x e32 from fp64 (allowed {T.FACTOR})"
    return r


@pytest.mark.parametrize("row", T.ROWS, ids=lambda r: r.name)
def test_adam_ema_twelve_steps(lib, row):
    p0, ema0 = T.params(T.N_ADAM)
    grads = T.grad_sequence(T.N_ADAM, T.STEPS)
    y = T.yardstick(row, p0, ema0, grads)
    got, sqs = device_run(lib, row, p0, ema0, grads)
    assert len(sqs) == (0 if row.max_norm is None else T.STEPS) and (got.ema is None) == (row.ema_beta is None)
    hold_to_yardstick(got, y, f"row {row.name}")


EDGE_N = [1, 255, 256, 257, 524288, 524289, 1200003]


@pytest.fixture(scope="module")
def whole(lib):
    """Two steps of row B on the largest buffers; the smaller sizes are prefixes of them."""
    n = max(EDGE_N)
    p0, ema0 = T.params(n)
    grads = T.grad_sequence(n, 2)
    got, sqs = device_run(lib, T.ROW["B"], p0, ema0, grads)
    return p0, ema0, grads, got, sqs


@pytest.mark.parametrize("n", EDGE_N)
def test_adam_ema_size_edges(lib, whole, n):
    row = T.ROW["B"]
    P0, E0, G, big, big_sqs = whole
    p0, ema0, grads = P0[:n].clone(), E0[:n].clone(), [g[:n].clone() for g in G]
    y = T.yardstick(row, p0, ema0, grads)
    got, _ = device_run(lib, row, p0, ema0, grads)
    hold_to_yardstick(got, y, f"n = {n}")
    # element i does not depend on n: with the whole buffer's norms, the prefix run leaves the bits of the whole run's prefix
    pre, _ = device_run(lib, row, p0, ema0, grads, sq_list=big_sqs)
    for k in range(2):
        assert torch.equal(pre.p_steps[k], big.p_steps[k][:n])
    assert torch.equal(pre.m, big.m[:n]) and torch.equal(pre.v, big.v[:n]) and torch.equal(pre.ema, big.ema[:n])
    # without an EMA buffer: the same p, exp_avg, exp_avg_sq
    bare, _ = device_run(lib, row, p0, ema0, grads, with_ema=False)
    assert bare.ema is None and torch.equal(bare.p_steps[1], got.p_steps[1]) and torch.equal(bare.m, got.m) and torch.equal(bare.v, got.v)


def test_adam_ema_empty_and_step_zero(lib):
    n = 300
    p0, ema0 = T.params(n)
    g = T.grad_sequence(n, 1)[0]
    m0, v0 = T.moments(n)
    bufs = [dev(t) for t in (p0, g, m0, v0, ema0)]
    keep = [t.clone() for t in bufs]
    # n == 0 through the C entry (an empty tensor has no pointer to hand over): OK, and nothing is touched
    rc = lib.load().mcedm_adam_ema_step(*(t.data_ptr() for t in bufs), 0, 1e-2, 0.8, 0.95, 1e-3, 1e-2, None, 1.0, 1.0, 0.99, 1, stream())
    torch.cuda.synchronize()
    assert rc == 0 and all(torch.equal(a, b) for a, b in zip(bufs, keep))
    with pytest.raises(RuntimeError, match="adam: step counts from 1"):
        lib.adam_ema_step(bufs[0], bufs[1], bufs[2], bufs[3], bufs[4], 0)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(bufs, keep))


@pytest.mark.parametrize("row", [T.ROW["A"], T.ROW["B"]], ids=lambda r: r.name)
def test_adam_ema_late_step(lib, row):
    """step = 100000 from given moments: beta^step (pow in double on the host) is 4e-44 at the most, both bias corrections are 1."""
    n, step = T.N_ADAM, 100000
    p0, ema0 = T.params(n)
    m0, v0 = T.moments(n)
    grads = T.grad_sequence(n, 1)
    y = T.yardstick(row, p0, ema0, grads, m0, v0, step - 1)
    got, _ = device_run(lib, row, p0, ema0, grads, m0, v0, step - 1)
    hold_to_yardstick(got, y, f"row {row.name} at step {step}")


# ------------------------------------------------------------------------------------------------ squared gradient norm
SQ_N = [0, 1, 255, 257, 524288, 524289, 1048577, 1572868]


def sq_input(n, seed=3):
    return torch.randn(max(n, 1), generator=T.gen(seed + n % 1000), dtype=torch.float32)[:n].clone()


def sq_bound(n):
    # every thread adds at most t non-negative fp32 terms into each of two accumulators (t - 1 roundings of a sum, one of each
    # square), the rest is fp64: (t + 2) U relative, with room for the two fp64 conversions
    return (T.sqnorm_terms(n) + 2) * U


@pytest.mark.parametrize("n", SQ_N)
def test_sqnorm(lib, n):
    scratch = fresh_scratch(lib)
    out = torch.full((1,), float("nan"), dtype=torch.float64, device="cuda")
    if n == 0:
        # through the C entry with a real pointer (an empty tensor has none): exactly 0.0 is written
        g = dev(sq_input(4))
        rc = lib.load().mcedm_sqnorm(g.data_ptr(), 0, out.data_ptr(), scratch.data_ptr(), scratch.numel(), stream())
        assert rc == 0 and float(out) == 0.0 and not bool(torch.signbit(out).any())
        return
    g = sq_input(n)
    ref = float((g.double() ** 2).sum())
    got = float(lib.sqnorm(dev(g), out, scratch=scratch))
    print(f"n = {n}: error / bound {abs(got - ref) / (sq_bound(n) * ref):.3f}")
    assert abs(got - ref) <= sq_bound(n) * ref
    again = float(lib.sqnorm(dev(g), scratch=scratch))          # the same scratch, not re-initialised
    assert again == got
    assert float(lib.sqnorm(dev(g), scratch=fresh_scratch(lib))) == got


def test_sqnorm_one_huge_element(lib):
    n = 524289
    g = sq_input(n)
    g[300001] = 1e15                    # its square is an fp32 number; the O(1) rest vanishes against it only in fp32 sums
    ref = float((g.double() ** 2).sum())
    got = float(lib.sqnorm(dev(g), scratch=fresh_scratch(lib)))
    assert abs(got - ref) <= sq_bound(n) * ref


def test_sqnorm_scratch_reuse_large_then_small(lib):
    """2048 blocks leave their partial sums in the scratch area; the next call, one block, must add slot 0 alone."""
    scratch = fresh_scratch(lib)
    big = sq_input(1572868)
    got = float(lib.sqnorm(dev(big), scratch=scratch))
    ref = float((big.double() ** 2).sum())
    assert abs(got - ref) <= sq_bound(big.numel()) * ref
    small = torch.tensor([1.7], dtype=torch.float32)
    assert float(lib.sqnorm(dev(small), scratch=scratch)) == float(small[0] * small[0])
    mid = sq_input(257)                  # two blocks after one
    ref = float((mid.double() ** 2).sum())
    assert abs(float(lib.sqnorm(dev(mid), scratch=scratch)) - ref) <= sq_bound(257) * ref


# ------------------------------------------------------------------------------------------------ losses
def loss_bound(shape):
    # a thread adds k non-negative terms in fp32 (k - 1 roundings), a term has three roundings of its own (the difference of the
    # masked values, its square, times the weight); the weight and the final cast to float make five; everything between is fp64
    return (T.loss_grid(shape)[1] + 5) * U


@pytest.mark.parametrize("mask_kind", ["binary", "fraction", "none"])
@pytest.mark.parametrize("sigma_data", [0.5, 1.0])
@pytest.mark.parametrize("shape", T.LOSS_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_edm_loss(lib, shape, sigma_data, mask_kind):
    D, x, m01, mfrac = T.loss_inputs(shape)
    mask = {"binary": m01, "fraction": mfrac, "none": None}[mask_kind]
    B = shape[0]
    m = torch.ones(shape, dtype=torch.float64) if mask is None else mask.double()
    for sigma in T.loss_sigmas(B):
        ref_loss, ref_dD = T.edm_loss_ref(D, x, mask, sigma, sigma_data)
        scratch = fresh_scratch(lib)
        loss, dD = lib.edm_loss(dev(D), dev(x), dev(mask), dev(sigma), sigma_data, scratch=scratch)
        assert loss.dtype == torch.float32 and tuple(dD.shape) == shape
        r_loss = abs(float(loss) - float(ref_loss)) / (loss_bound(shape) * float(ref_loss))
        # relative to the operands, not to the difference, which cancels where D is close to x
        w = T.edm_weight(sigma, sigma_data).view(-1, 1, 1, 1)
        lim = 8 * U * (2 * w / B) * ((D.double() * m).abs() + (x.double() * m).abs()) * m.abs()
        r_dD = ratio(dD, ref_dD, lim)
        print(f"edm_loss {shape} sigma {float(sigma[0]):g}..{float(sigma[-1]):g} sigma_data {sigma_data} mask {mask_kind}: "
              f"error / bound: loss {r_loss:.3f}, dD {r_dD:.3f}")
        assert r_loss <= 1 and r_dD <= 1
        only, none = lib.edm_loss(dev(D), dev(x), dev(mask), dev(sigma), sigma_data, want_grad=False, scratch=scratch)
        assert none is None and torch.equal(only, loss)
        if B == 65:                      # more than one block per sample, more samples than a wave: the order is fixed
            again, dD2 = lib.edm_loss(dev(D), dev(x), dev(mask), dev(sigma), sigma_data, scratch=fresh_scratch(lib))
            assert torch.equal(again, loss) and torch.equal(dD2, dD)


@pytest.mark.parametrize("shape", T.LOSS_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_eps_loss(lib, shape):
    F, eps = T.loss_inputs(shape)[:2]
    B = shape[0]
    ref_loss, ref_dF = T.eps_loss_ref(F, eps)
    scratch = fresh_scratch(lib)
    loss, dF = lib.eps_loss(dev(F), dev(eps), scratch=scratch)
    r_loss = abs(float(loss) - float(ref_loss)) / (loss_bound(shape) * float(ref_loss))
    r_dF = ratio(dF, ref_dF, 4 * U * (2.0 / B) * (F.double().abs() + eps.double().abs()))
    print(f"eps_loss {shape}: error / bound: loss {r_loss:.3f}, dF {r_dF:.3f}")
    assert r_loss <= 1 and r_dF <= 1
    only, none = lib.eps_loss(dev(F), dev(eps), want_grad=False, scratch=scratch)
    assert none is None and torch.equal(only, loss)
    if B == 65:
        again, dF2 = lib.eps_loss(dev(F), dev(eps), scratch=fresh_scratch(lib))
        assert torch.equal(again, loss) and torch.equal(dF2, dF)


def test_losses_reject_a_batch_beyond_the_reduction_table(lib):
    shape = (4097, 1, 1, 1)
    a, b, s = torch.ones(shape).cuda(), torch.zeros(shape).cuda(), torch.ones(4097).cuda()
    with pytest.raises(RuntimeError, match="exceeds the reduction table"):
        lib.edm_loss(a, b, None, s)
    with pytest.raises(RuntimeError, match="exceeds the reduction table"):
        lib.eps_loss(a, b)
    # 4096 is the last batch the table takes: loss = mean_b 2 (1 - 0)^2
    loss, dD = lib.edm_loss(a[:4096].contiguous(), b[:4096].contiguous(), None, s[:4096].contiguous())
    assert float(loss) == 2.0 and bool((dD == 2 * 2.0 / 4096).all())


# ------------------------------------------------------------------------------------------------ noise inputs
@pytest.mark.parametrize("shape", [(3, 2, 5, 7), (5, 2, 231, 229)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("P", [(-1.2, 1.2), (0.3, 0.7)], ids=["default", "0.3_0.7"])
@pytest.mark.parametrize("masked", [True, False])
def test_edm_noise_inputs(lib, shape, P, masked):
    B = shape[0]
    assert shape == (3, 2, 5, 7) or B * shape[1] * shape[2] * shape[3] > 524288          # one sweep of the capped grid
    g = T.gen(11)
    x, noise = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
    mask = (torch.rand(shape, generator=g) < 0.5).float() * 0.75 if masked else None
    rnd = torch.linspace(-3.0, 3.0, B)
    args = (dev(x), dev(mask), dev(noise), dev(rnd))
    x_noise, sigma = lib.edm_noise_inputs(*args) if P == (-1.2, 1.2) else lib.edm_noise_inputs(*args, P_mean=P[0], P_std=P[1])
    # two roundings of an argument of magnitude <= 6 (6 x 2 U = 7e-7) and 2 ulp of expf (2.4e-7) come to 1e-6: twice that
    torch.testing.assert_close(sigma.cpu().double(), (rnd.double() * P[1] + P[0]).exp(), rtol=2e-6, atol=0)
    s = sigma.cpu().double().view(-1, 1, 1, 1)
    mn = noise.double() if mask is None else mask.double() * noise.double()
    r = ratio(x_noise, x.double() + mn * s, 4 * U * (x.double().abs() + (mn * s).abs()))
    print(f"edm_noise_inputs {shape} P {P} masked {masked}: error / bound {r:.3f}")
    assert r <= 1


def eps_case(shape_x, seed=21):
    B = shape_x[0]
    g = T.gen(seed)
    x, noise, F0 = (torch.randn(shape_x, generator=g) for _ in range(3))
    t = torch.tensor([0, 999, 417] + [123] * (B - 3), dtype=torch.int64)[:B]
    return x, noise, F0, t


def test_eps_noise_inputs(lib):
    a, b = T.ddpm_tables(1000)
    x, noise, _, t = eps_case((3, 2, 5, 7))
    x_noise, labels = lib.eps_noise_inputs(dev(x), dev(noise), dev(t), dev(a), dev(b))
    assert labels.dtype == torch.float32 and torch.equal(labels.cpu(), t.float())
    at, bt = a[t].double().view(-1, 1, 1, 1), b[t].double().view(-1, 1, 1, 1)
    # two products and their sum: three roundings, each of at most U x (|x a| + |n b|)
    r = ratio(x_noise, x.double() * at + noise.double() * bt, 3 * U * ((x.double() * at).abs() + (noise.double() * bt).abs()))
    print(f"eps_noise_inputs: error / bound {r:.3f}")
    assert r <= 1
    with pytest.raises(RuntimeError, match="timesteps outside"):
        lib.eps_noise_inputs(dev(x), dev(noise), dev(torch.tensor([0, 1000, 1])), dev(a), dev(b))


# (cond channels, cond given, F0 given): the four combinations, and no cond channels at all
@pytest.mark.parametrize("cond_ch,with_cond,with_F0", [(2, True, True), (2, True, False), (2, False, True), (2, False, False),
                                                       (0, False, True), (0, False, False)])
def test_eps_self_cond(lib, cond_ch, with_cond, with_F0):
    a, b = T.ddpm_tables(1000)
    B, in_ch, H, W = 3, 2, 5, 7
    x, noise, F0, t = eps_case((B, in_ch, H, W))
    at, bt = a[t].view(-1, 1, 1, 1), b[t].view(-1, 1, 1, 1)
    x_noise = x * at + noise * bt
    cond = torch.randn((B, cond_ch, H, W), generator=T.gen(5)) if with_cond else None
    out = torch.full((B, cond_ch + in_ch, H, W), float("nan"), device="cuda")
    kw = dict(x_noise=dev(x_noise), F0=dev(F0), t=dev(t), sqrt_ab=dev(a), sqrt_1mab=dev(b)) if with_F0 else {}
    got = lib.eps_self_cond(out, dev(cond), cond_ch, in_ch, **kw).cpu()
    assert not bool(torch.isnan(got).any())
    assert torch.equal(got[:, :cond_ch], cond if with_cond else torch.zeros(B, cond_ch, H, W))
    sc = got[:, cond_ch:]
    if not with_F0:
        assert bool((sc == 0).all())
        return
    ad, bd = at.double(), bt.double()
    ref = (x_noise.double() - F0.double() * bd) / ad
    # the product, the difference and the quotient: three roundings of at most U x (|x_noise| + |F0 b|) / a, and one to spare
    r = ratio(sc, ref, 4 * U * (x_noise.double().abs() + (F0.double() * bd).abs()) / ad)
    print(f"eps_self_cond cond {with_cond} cond_ch {cond_ch}: error / bound {r:.3f}")
    assert r <= 1


# ------------------------------------------------------------------------------------------------ FusedAdamEma
def toy():
    torch.manual_seed(0)
    return torch.nn.Sequential(torch.nn.Linear(7, 13), torch.nn.Linear(13, 3))


@pytest.mark.parametrize("max_norm", [1.0, None], ids=["clip", "noclip"])
def test_fused_adam_ema_against_torch(lib, max_norm):
    import copy
    from mcedm_amd.optim import FusedAdamEma
    row = T.Row("toy", 1e-2, 0.8, 0.95, 1e-8, 1e-2, max_norm, 1.0, 0.99)
    net = toy()
    shapes = [tuple(p.shape) for p in net.parameters()]
    sizes = [p.numel() for p in net.parameters()]
    n, steps = sum(sizes), 10
    assert n == 146
    p0s = [p.detach().clone() for p in net.parameters()]
    flat_g = T.grad_sequence(n, steps)
    grads = [[c.view(s) for c, s in zip(g.split(sizes), shapes)] for g in flat_g]
    lr_at = lambda k: row.lr if k < 5 else 0.5 * row.lr                           # noqa: E731
    # the reference: torch.optim.Adam + clip_grad_norm_ + the EMA formula on an fp64 CPU copy; the yardstick: the same in fp32
    ref = T.torch_run(row, torch.float64, p0s, p0s, grads, lr_at=lr_at)
    y = T.against(ref, T.torch_run(row, torch.float32, p0s, p0s, grads, lr_at=lr_at), torch.cat([p.flatten() for p in p0s]))
    net = net.cuda()
    ema_net = copy.deepcopy(net)
    opt = FusedAdamEma(net, ema_net, lr=row.lr, betas=(row.b1, row.b2), weight_decay=row.wd, ema_beta=row.ema_beta, max_norm=max_norm)
    ps = []
    for k in range(steps):
        if k == 5:
            opt.param_groups[0]["lr"] *= 0.5         # as a scheduler does
        for p, g in zip(net.parameters(), grads[k]):
            p.grad = g.cuda()
        opt.step()
        ps.append(torch.cat([p.detach().flatten() for p in net.parameters()]).cpu())
        if max_norm is None:
            assert opt.last_grad_norm is None
        else:
            want = float((flat_g[k].double() ** 2).sum())
            assert abs(float(opt.last_grad_norm) - want) <= sq_bound(n) * want
    got = T.Run(ps, opt.flat_m.cpu(), opt.flat_v.cpu(), torch.cat([p.detach().flatten() for p in ema_net.parameters()]).cpu())
    hold_to_yardstick(got, y, f"FusedAdamEma max_norm {max_norm}")
    st = opt.state_dict()["state"]
    assert len(st) == 4 and all(float(s["step"]) == steps for s in st.values())
