"""GPU: the PDE term of training (optimization.pde_loss_lambda > 0, models/ddim.py:1726-1731) on the HIP path:
mcedm_pde_train_loss through ``lib.pde_train_loss`` against the reference's get_pde_loss (tests/golden/pde_train.npz) and the float64
restatement of tests/_pde_train.py, and ``PlCondEdm.training_step`` with the term against the reference's training runs.  The bar is
the project's: rtol 1e-4, atol 1e-5 max|ref| (tests/test_pde.py::_close_grad, tests/test_hip_backward.py)."""
import ctypes as C

import pytest
import torch

from oracle import fixtures as fx
from oracle import mcedm_oracle as orc
from tests import _ddpm_edm as DD
from tests import _pde_train as T
from tests.test_hip_cond_edm import cond_hparams
from tests.test_hip_module import wrap

pytestmark = pytest.mark.gpu
LAM = 0.37            # op level: any factor; the fixture holds the gradient of the term itself


def desc(c, lam=LAM, stats=None):
    from mcedm_amd.pde_loss import get_pde_loss_function
    from mcedm_amd.pl_base import Normalizer
    st = stats or c["stats"]
    nh, nu = Normalizer(()), Normalizer(())
    nh.set_stats(torch.tensor(st[0]), torch.tensor(st[1]))
    nu.set_stats(torch.tensor(st[2]), torch.tensor(st[3]))
    return get_pde_loss_function(c["system"], False)[0].guidance_desc(nh, nu, c["H"], c["W"], weight=lam)


def dev_inputs(name):
    h, D, gt, sigma = T.op_inputs(name)
    w = None if sigma is None else T.sample_weights(sigma.cuda())
    return h.cuda(), D.cuda(), None if gt is None else gt.cuda(), w


def close_grad(got, ref, what):
    """tests/test_pde.py::_close_grad with rtol 1e-4: atol 1e-5 max|ref|; what the reference zeroes is zero, its NaNs are NaNs."""
    got, ref = got.detach().cpu().double(), torch.as_tensor(ref).double()
    scale = float(ref.nan_to_num().abs().max())
    err = float((got - ref).nan_to_num().abs().max())
    print(f"{what}: max|d| = {err:.3e} on max|ref| = {scale:.3e}")
    torch.testing.assert_close(got, ref, rtol=1e-4, atol=1e-5 * scale, equal_nan=True,
                               msg=lambda m: f"{what}: {m}")
    assert bool((got == 0)[ref == 0].all()), f"{what}: entries that are exactly zero in the reference must be exactly zero"


@pytest.mark.parametrize("name", list(T.OP_CASES))
def test_value_and_gradient_golden(golden, name):
    from mcedm_amd import lib as L
    g = golden("pde_train.npz")
    c = T.OP_CASES[name]
    h, D, gt, w = dev_inputs(name)
    val, dD = L.pde_train_loss(desc(c, 1.0), D, h, gt=gt, w=w, dD=torch.zeros_like(D))
    ref_v, ref_g = torch.as_tensor(g[f"{name}::value"]), torch.as_tensor(g[f"{name}::grad"])
    print(f"{name}: value {float(val):.6f} vs {float(ref_v):.6f}")
    torch.testing.assert_close(val.cpu().reshape(()), ref_v, rtol=1e-4, atol=0, equal_nan=True)
    close_grad(dD, ref_g, f"{name} vs the reference")
    if c["dry"]:
        return          # in float64 h + 1e-8 is not 0: the restatement describes another state there
    v64, g64 = T.restate(c["system"], *T.op_inputs(name), dtype=torch.float64, stats=c["stats"])
    torch.testing.assert_close(val.cpu().reshape(()).double(), v64, rtol=1e-4, atol=0)
    close_grad(dD, g64, f"{name} vs float64")


@pytest.mark.parametrize("name", ["swe_per_5x7x37_self_propt", "swe_2x3x3_gt", "darcy_S19_propt"])
def test_gradient_accumulates_and_null_is_the_value_alone(name):
    from mcedm_amd import lib as L
    c = T.OP_CASES[name]
    h, D, gt, w = dev_inputs(name)
    v1, g1 = L.pde_train_loss(desc(c, 1.0), D, h, gt=gt, w=w, dD=torch.zeros_like(D))
    pattern = torch.arange(D.numel(), dtype=torch.float32, device="cuda").reshape(D.shape).sin()
    v2, g2 = L.pde_train_loss(desc(c, LAM), D, h, gt=gt, w=w, dD=pattern.clone())
    v3, none = L.pde_train_loss(desc(c, LAM), D, h, gt=gt, w=w)
    assert none is None and torch.equal(v1, v2) and torch.equal(v1, v3)          # the value is not multiplied by lambda
    ref = pattern.double() + LAM * g1.double()
    torch.testing.assert_close(g2.double(), ref, rtol=1e-6, atol=1e-6 * float(ref.abs().max()))
    assert torch.equal(g2[g1 == 0], pattern[g1 == 0])


def test_h_is_read_in_place_through_its_strides():
    """training_step holds h as a channel slice of the normalised (b, h, w, 2) batch."""
    from mcedm_amd import lib as L
    name = "swe_per_3x8x16_self"
    c = T.OP_CASES[name]
    h, D, gt, w = dev_inputs(name)
    x = torch.cat([h, torch.full_like(h, 7.0)], dim=-1)
    ref = L.pde_train_loss(desc(c), D, h, dD=torch.zeros_like(D))
    got = L.pde_train_loss(desc(c), D, x[..., 0:1], dD=torch.zeros_like(D))
    assert not x[..., 0:1].is_contiguous() and torch.equal(ref[0], got[0]) and torch.equal(ref[1], got[1])


@pytest.mark.parametrize("name", ["swe_5x7x37_gt_propt", "darcy_S19"])
def test_two_runs_are_bit_equal(name):
    from mcedm_amd import lib as L
    c = T.OP_CASES[name]
    h, D, gt, w = dev_inputs(name)
    runs = [L.pde_train_loss(desc(c), D, h, gt=gt, w=w, dD=torch.ones_like(D)) for _ in range(2)]
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


def test_argument_errors_name_the_argument_and_launch_nothing():
    from mcedm_amd import lib as L
    lib = L.load()
    swe, darcy = T.OP_CASES["swe_per_3x8x16_self"], T.OP_CASES["darcy_S8"]
    B, H, W = 3, 8, 16
    D = torch.zeros(B, 1, H, W, device="cuda")
    h = torch.zeros(B, H, W, device="cuda")
    loss = torch.full((1,), -3.0, device="cuda")
    dD = torch.full_like(D, 5.0)
    red = L.reduce_scratch("cuda")
    G = torch.zeros(B * 16, device="cuda")

    def call(gd, **over):
        a = dict(gd=C.byref(gd) if gd is not None else None, D=D.data_ptr(), h=h.data_ptr(), B=B, H=H, W=W, loss=loss.data_ptr(),
                 dD=dD.data_ptr(), G=G.data_ptr(), Gb=G.numel() * 4, red=red.data_ptr(), redb=red.numel())
        a.update(over)
        rc = lib.mcedm_pde_train_loss(a["gd"], a["D"], a["h"], H * W, W, 1, None, None, a["B"], a["H"], a["W"], a["loss"], a["dD"],
                                      a["G"], a["Gb"], a["red"], a["redb"], L._stream())
        return rc, lib.mcedm_last_error().decode()

    bad = desc(swe)
    bad.system = 7
    cases = [(call(None), "gd is null"), (call(desc(swe), D=None), "D is null"), (call(desc(swe), h=None), "h is null"),
             (call(desc(swe), loss=None), "loss_out is null"), (call(bad), "gd->system = 7 is unknown"),
             (call(desc(swe), B=0), "empty shape"), (call(desc(swe), red=None), "scratch needs"),
             (call(desc(swe), redb=64), "scratch needs"),
             (call(desc(darcy)), "Darcy needs a square grid (H = 8, W = 16)"),
             (call(desc(darcy), H=4, W=4), "larger than 4 x 4 (S = 4)"),
             (call(desc(darcy), H=8, W=8, G=None), "pde_scratch needs 192 bytes"),
             (call(desc(darcy), H=8, W=8, Gb=191), "pde_scratch needs 192 bytes")]
    for (rc, msg), want in cases:
        assert rc == L.abi.CONSTS["MCEDM_ERR_INVALID"] and want in msg, (rc, msg, want)
    torch.cuda.synchronize()
    assert float(loss) == -3.0 and bool((dD == 5.0).all())
    assert lib.mcedm_pde_train_scratch_bytes(C.byref(desc(darcy)), 3, 8, 8) == 3 * 16 * 4
    assert lib.mcedm_pde_train_scratch_bytes(C.byref(desc(swe)), 3, 8, 16) == 0


# ---- PlCondEdm.training_step with the term -------------------------------------------------------------------------------
def make_module(golden, system, lam, use_gt=False, prop_t=False):
    import mcedm_amd  # noqa: F401
    from mcedm_amd.ddim import PlCondEdm
    hp = cond_hparams()
    hp.model.cond_p = T.COND_P
    hp.optimization.update(pde_loss_lambda=lam, use_gt_pde=use_gt, pde_loss_prop_t=prop_t)
    m = PlCondEdm(hp).cuda()
    P = orc.make_params(fx.CFG_C, T.MODULE_SEED)
    with torch.no_grad():
        for net in (m.model, m.ema_model.ma_model):
            for n, p in net.named_parameters():
                p.copy_(P[n])
    st = T.module_inputs(system)[4]
    m.normalizer_input.set_stats(torch.tensor(st[0]), torch.tensor(st[1]))
    m.normalizer_target.set_stats(torch.tensor(st[2]), torch.tensor(st[3]))
    m.set_pde_loss_function(system, False)
    m.logged = {}
    m.log = lambda k, v, **kw: m.logged.__setitem__(k, v.detach().clone())
    return m


def run_step(m, monkeypatch, system, r_cond):
    h, u, noise, rnd_normal, _ = T.module_inputs(system)
    rands = [r_cond]
    with monkeypatch.context() as mp:
        mp.setattr(torch, "randn_like", lambda t, **k: noise.cuda())
        mp.setattr(torch, "randn", lambda *a, **k: rnd_normal)
        mp.setattr(torch, "rand", lambda *a, **k: torch.tensor([rands.pop(0)]))
        loss = m.training_step((h.cuda(), None, None, u.cuda()), 0)
    assert not rands
    return loss


def close(got, ref, rtol=1e-4, atol=1e-5):
    torch.testing.assert_close(got.detach().cpu(), torch.as_tensor(ref), rtol=rtol, atol=atol)


@pytest.mark.parametrize("tag", list(T.MODULE_CASES))
def test_training_step_golden(golden, monkeypatch, tag):
    """Loss, both logged parts, named gradients and every parameter's squared norm against the reference's training_step run with
    get_pde_loss fed as its evaluation loops feed it (see tools/make_golden_pde_train.py: as written, :1729 raises)."""
    g = golden("pde_train.npz")
    system, use_gt, prop_t, r_cond = T.MODULE_CASES[tag]
    m = make_module(golden, system, float(g[f"{tag}::lambda"]), use_gt, prop_t)
    loss = run_step(m, monkeypatch, system, r_cond)
    assert loss.dtype == torch.float32
    loss.backward()
    for key, got in (("loss", loss), ("train_loss", m.logged["train_loss"]), ("train_pde_loss", m.logged["train_pde_loss"])):
        print(f"{tag} {key}: {float(got.detach()):.6f} vs {float(g[f'{tag}::{key}']):.6f}")
        close(got, g[f"{tag}::{key}"], rtol=1e-4, atol=0)
    grads = {n: p.grad for n, p in m.model.named_parameters()}
    for n in T.MODULE_GRAD_NAMES:
        ref = torch.as_tensor(g[f"{tag}::grad::{n}"])
        print(f"{tag} {n}: max|d| = {float((grads[n].cpu() - ref).abs().max()):.3e} on max|ref| = {float(ref.abs().max()):.3e}")
        close(grads[n], ref, rtol=1e-4, atol=1e-5 * float(ref.abs().max()))
    sq = torch.tensor([float((gr.double() ** 2).sum()) for gr in grads.values()])
    ref_sq = torch.as_tensor(g[f"{tag}::grad_sqnorm_each"])
    torch.testing.assert_close(sq, ref_sq, rtol=2e-4, atol=1e-10 * float(ref_sq.max()))          # squared: twice the bar


def test_two_optimizer_steps_golden(golden, monkeypatch):
    g = golden("pde_train.npz")
    m = make_module(golden, "swe_per", float(g["swe_self::lambda"]))
    opt = m.configure_optimizers()["optimizer"]
    for step, r_cond in enumerate(T.OPT_DRAWS):
        opt.zero_grad()
        loss = run_step(m, monkeypatch, "swe_per", r_cond)
        loss.backward()
        m.configure_gradient_clipping(opt, 1.0, "norm")
        m.optimizer_step(0, 0, opt, 0, lambda: loss)
        close(loss, g[f"opt::loss{step}"], rtol=1e-4, atol=0)
    pn, en = dict(m.model.named_parameters()), dict(m.ema_model.ma_model.named_parameters())
    for n in T.MODULE_GRAD_NAMES:
        close(pn[n], g[f"opt::param::{n}"], rtol=1e-4, atol=2e-6)
        close(en[n], g[f"opt::ema::{n}"], rtol=1e-5, atol=1e-6)


def test_training_step_is_bitwise_reproducible(golden, monkeypatch):
    g = golden("pde_train.npz")
    out = []
    for _ in range(2):
        m = make_module(golden, "swe_per", float(g["swe_propt::lambda"]), prop_t=True)
        loss = run_step(m, monkeypatch, "swe_per", 0.1)
        loss.backward()
        out.append((loss.detach().clone(), m.logged["train_pde_loss"], [p.grad.clone() for p in m.model.parameters()]))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    assert all(torch.equal(a, b) for a, b in zip(out[0][2], out[1][2]))


def test_lambda_zero_never_calls_the_entry(golden, monkeypatch):
    """The step of a module without the term is today's: the new binding is not called, and the loss and gradients are the cond_edm
    golden's."""
    from mcedm_amd import lib as L
    g = golden("cond_edm.npz")
    m = make_module(golden, "swe_per", 0.0)
    h, u, noise, rnd_normal = fx.cond_training_inputs()

    def refuse(*a, **k):
        raise AssertionError("pde_train_loss called with pde_loss_lambda == 0")
    monkeypatch.setattr(L, "pde_train_loss", refuse)
    monkeypatch.setattr(torch, "randn_like", lambda t, **k: noise.cuda())
    monkeypatch.setattr(torch, "randn", lambda *a, **k: rnd_normal)
    monkeypatch.setattr(torch, "rand", lambda *a, **k: torch.tensor([0.1]))
    loss = m.training_step((h.cuda(), None, None, u.cuda()), 0)
    monkeypatch.undo()
    assert set(m.logged) == {"train_loss"}
    close(loss, torch.as_tensor(g["loss"]), rtol=1e-4, atol=1e-4)
    loss.backward()
    grads = dict(m.model.named_parameters())
    for n in fx.COND_GRAD_NAMES:
        ref = torch.as_tensor(g[f"grad::{n}"])
        close(grads[n].grad, ref, rtol=1e-4, atol=1e-5 * float(ref.abs().max()))


@pytest.mark.parametrize("what", ["flip_xy", "min_max", "rescaled", "two_channels", "no_pde_loss"])
def test_unbuilt_forms_raise_in_training_step(golden, monkeypatch, what):
    m = make_module(golden, "swe_per", 0.1)
    h, u, _, _, _ = T.module_inputs("swe_per")
    err, match = NotImplementedError, what
    if what == "flip_xy":
        m.set_pde_loss_function("swe_per", True)
    elif what == "min_max":
        m.normalization = "min_max"
    elif what == "rescaled":
        m.rescaled = True
    elif what == "two_channels":
        h, u, match = torch.cat([h, h], dim=-1), torch.cat([u, u], dim=-1), "more than one channel"
    else:
        m.pde_loss, err, match = None, RuntimeError, "set_pde_loss_function"
    with pytest.raises(err, match=match):
        m.training_step((h.cuda(), None, None, u.cuda()), 0)


def test_ddpm_unet_adds_the_term_under_no_grad_and_still_refuses_to_train(monkeypatch):
    import mcedm_amd  # noqa: F401
    from mcedm_amd import lib as L
    from mcedm_amd.ddim import PlCondEdm
    lam = 0.25
    hd = DD.hparams_dict()
    hd["optimization"].update(pde_loss_lambda=lam)
    m = DD.fill(PlCondEdm(wrap(hd)).cuda(), 1, fx.TRAIN_NORM_STATS)
    m.set_pde_loss_function("swe_per", False)
    m.logged = {}
    m.log = lambda k, v, **kw: m.logged.__setitem__(k, v.detach().clone())
    seen = {}
    real = L.pde_train_loss

    def spy(gd, D, h, **kw):
        seen["D"], seen["dD"] = D.clone(), kw.get("dD")
        return real(gd, D, h, **kw)
    monkeypatch.setattr(L, "pde_train_loss", spy)
    with torch.no_grad():
        loss = run_step(m, monkeypatch, "swe_per", 0.1)
    assert seen["dD"] is None
    h, u, _, _, st = T.module_inputs("swe_per")
    c = dict(system="swe_per", H=32, W=32)
    pde = real(desc(c, lam, st), seen["D"], m.data_transform(h.cuda(), u.cuda())[..., 0:1])[0].reshape(())
    assert torch.equal(m.logged["train_pde_loss"], pde)
    assert torch.equal(loss, m.logged["train_loss"] + lam * pde) and float(pde) > 0
    with pytest.raises(NotImplementedError, match="not built on the DDPM U-Net"):
        run_step(m, monkeypatch, "swe_per", 0.1)
