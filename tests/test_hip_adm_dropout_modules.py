"""GPU: hparams.model.dropout through the drop-in modules on the ADM U-Net -- PlMcedm, PlCondEdm, and PlCondDdim with dx_cond
(cat_dx: the ``_dx`` entries) -- at 32 x 32.

train(): ``training_step`` with ``_draw_seed`` patched to a constant equals, at the project's bar, the fp64 oracle with the device
generator's masks injected (tests/_adm_dropout.py) evaluated on the very tensors the module handed to its fused loss; the step's
other draws (noise, rnd_normal / t, the dx / cond_p / self-conditioning rands) are those of a dropout = 0 module under the same
torch.manual_seed.  eval(): ``training_step``'s loss and gradients and the samplers are bit-identical to the dropout = 0 module
with the same weights.  The flat trainer's step equals the module path bit for bit at the same seed.
"""
import contextlib

import pytest
import torch

from oracle import fixtures as fx
from oracle import mcedm_oracle as orc
from tests import _adm_arch as A
from tests import _adm_dropout as D
from tests import _cond_dx as X
from tests.test_cond_ddim_cpu import ddim_hparams
from tests.test_hip_cond_ddim import train_inputs as ddim_train_inputs
from tests.test_hip_cond_edm import cond_hparams
from tests.test_hip_module import hparams

pytestmark = pytest.mark.gpu

P = D.P_DROP
SEED = 0x1234567890ABCDE
KINDS = ("mcedm", "cond_edm", "cond_ddim_dx")


def make(kind, dropout):
    import mcedm_amd  # noqa: F401
    from mcedm_amd.ddim import PlCondDdim, PlCondEdm
    from mcedm_amd.mcedm import PlMcedm
    if kind == "mcedm":
        hp, cls, cfg, seed, st = hparams(fx.CFG_P), PlMcedm, fx.CFG_P, 7, fx.TRAIN_NORM_STATS
    elif kind == "cond_edm":
        hp, cls, cfg, seed, st = cond_hparams(), PlCondEdm, fx.CFG_C, 11, fx.TRAIN_NORM_STATS
    else:
        hp, cls, cfg, seed, st = ddim_hparams(**X.model_update("cat")), PlCondDdim, X.cfg_of("cat"), X.SEED, fx.TRAIN_NORM_STATS
        hp.model.dx_cond = True
    hp.model.dropout = dropout
    m = cls(hp).cuda()
    Pm = orc.make_params(cfg, seed)
    assert [n for n, _ in m.model.named_parameters()] == list(Pm)
    with torch.no_grad():
        for mod in (m.model, m.ema_model.ma_model):
            for n, p in mod.named_parameters():
                p.copy_(Pm[n])
    m.normalizer_input.set_stats(torch.tensor(st[0]).cuda(), torch.tensor(st[1]).cuda())
    m.normalizer_target.set_stats(torch.tensor(st[2]).cuda(), torch.tensor(st[3]).cuda())
    if kind == "cond_ddim_dx":
        m.set_pde_loss_function("swe_per", False)
    m.log = lambda *a, **k: None
    return m, cfg


def batch(kind):
    if kind == "mcedm":
        h, u, mask, _, _, _ = fx.training_inputs()
        return (h.cuda(), None, None, u.cuda(), mask.cuda())
    if kind == "cond_edm":
        h, u, _, _ = fx.cond_training_inputs()
        return (h.cuda(), None, None, u.cuda())
    h, u, _, _ = ddim_train_inputs()
    return (h, None, None, u)


@contextlib.contextmanager
def captured(monkeypatch, seed=SEED):
    """Records what training_step hands to its fused loss, and pins the dropout seed."""
    import mcedm_amd  # noqa: F401
    from mcedm_amd import ddim, mcedm, pl_base
    got = {}
    edm, eps = mcedm._edm_train_loss, ddim._eps_train_loss

    def edm_loss(module, x, x_noise, sigma, cond, mask, dx, extra=None):
        got.update(kind="edm", x=x, x_noise=x_noise, sigma=sigma, cond=cond, mask=mask, dx=dx)
        return edm(module, x, x_noise, sigma, cond, mask, dx, extra)

    def eps_loss(module, x_noise, labels, cond, noise, dx=None):
        got.update(kind="eps", x_noise=x_noise, labels=labels, cond=cond, noise=noise, dx=dx)
        return eps(module, x_noise, labels, cond, noise, dx)

    with monkeypatch.context() as mp:
        mp.setattr(mcedm, "_edm_train_loss", edm_loss)
        mp.setattr(ddim, "_edm_train_loss", edm_loss)
        mp.setattr(ddim, "_eps_train_loss", eps_loss)
        if seed is not None:
            mp.setattr(pl_base._PlBase, "_draw_seed", staticmethod(lambda: seed))
        yield got


def step(m, kind, monkeypatch, manual_seed=1234, pin=True):
    """One training_step + backward under torch.manual_seed -> (loss, name -> gradient, what the fused loss was handed, the next
    torch.rand(1) behind the step).  pin=False: the dropout seed is drawn from torch's generator, as in production."""
    m.zero_grad()
    with captured(monkeypatch, SEED if pin else None) as got:
        torch.manual_seed(manual_seed)
        loss = m.training_step(batch(kind), 0)
        after = torch.rand(1)                     # the generator's state behind the step
    loss.backward()
    return loss.detach().clone(), {n: p.grad.detach().clone() for n, p in m.model.named_parameters()}, dict(got), after


def oracle64(net, got, masks):
    """Loss and gradients of the fp64 oracle with the masks injected, on the tensors the fused loss was handed."""
    a = net._arch
    from mcedm_amd import lib as L
    mode = "" if a["dx_mode"] == L.DX_NONE else ("cat" if a["dx_mode"] == L.DX_CAT else "enc")
    cfg = orc.UNetConfig(in_channels=a["in_channels"], cond_channels=a["cond_channels"], out_ch=a["out_channels"], ch=a["ch"],
                         ch_mult=tuple(a["ch_mult"]), num_res_blocks=a["num_res_blocks"], attn_resolutions=tuple(a["attn_resolutions"]),
                         resolution=a["resolution"], dx_channels=a["dx_channels"], dx_mode=mode)
    Pm = {n: p.detach().cpu().double().requires_grad_(True) for n, p in net.named_parameters()}
    t = {k: (v.detach().cpu().double() if torch.is_tensor(v) else v) for k, v in got.items()}
    with D.injected(Pm, masks, P) as hits:
        if got["kind"] == "edm":
            sigma = t["sigma"].reshape(-1, 1, 1, 1)
            c_skip, c_out, c_in, c_noise = orc.precond_coeffs(sigma)
            F = orc.unet_forward(Pm, cfg, c_in * t["x_noise"], c_noise.flatten(), t["cond"], dx=t["dx"])
            Dn = c_skip * t["x_noise"] + c_out * F
            m = torch.ones_like(Dn) if t["mask"] is None else t["mask"]
            loss = (orc.loss_weight(sigma) * (Dn * m - t["x"] * m) ** 2).sum(dim=(1, 2, 3)).mean()
        else:
            F = orc.unet_forward(Pm, cfg, t["x_noise"], t["labels"], t["cond"], dx=t["dx"])
            loss = ((F - t["noise"]) ** 2).sum(dim=(1, 2, 3)).mean()
    assert sorted(hits) == sorted(masks)
    return loss.detach(), dict(zip(Pm, torch.autograd.grad(loss, list(Pm.values())))), cfg


@pytest.mark.parametrize("kind", KINDS)
def test_training_step_in_train_and_eval_mode(kind, monkeypatch):
    from mcedm_amd import lib as L
    from tests.test_hip_adm_dropout import seed_tensor
    m0, _ = make(kind, 0.0)
    m, _ = make(kind, P)
    assert m.model.dropout == P and m.model.training
    plain = step(m0, kind, monkeypatch)
    assert m0.model._drop_seed is None                                    # p = 0: nothing drawn, nothing allocated
    # ---- train(): against the fp64 oracle with the device generator's masks
    loss, grads, got, after = step(m, kind, monkeypatch)
    for k in ("x_noise", "sigma", "labels", "noise", "cond", "dx", "x"):      # the reference-ordered draws are the p = 0 module's
        a, b = got.get(k), plain[2].get(k)
        assert (a is None and b is None) or torch.equal(a, b), k
    if kind == "cond_ddim_dx":
        assert got["dx"] is not None and got["cond"] is not None          # the _dx entries and the conditioned branch ran
    B, _, H, W = got["x_noise"].shape
    a = m.model._arch
    st = seed_tensor(SEED)
    shapes = D.block_shapes(orc.UNetConfig(in_channels=a["in_channels"], cond_channels=a["cond_channels"], out_ch=a["out_channels"],
                                           ch=a["ch"], ch_mult=tuple(a["ch_mult"]), num_res_blocks=a["num_res_blocks"],
                                           attn_resolutions=tuple(a["attn_resolutions"]), resolution=a["resolution"]), B, H, W)
    masks = {key: D.keep_device(L, st, j, shape, P) for j, (key, shape) in enumerate(shapes)}
    loss64, g64, _ = oracle64(m.model, got, masks)
    r_l = A.bar_ratio(loss.reshape(1), loss64.reshape(1))
    r_g, n_g = max((A.bar_ratio(grads[n], g64[n]), n) for n in grads if float(g64[n].abs().max()) > 0)
    zero = [n for n in grads if float(g64[n].abs().max()) == 0]
    assert all(float(grads[n].abs().max()) == 0 for n in zero), zero
    print(f"{kind} [dropout {P}]: worst err / bar vs the fp64 oracle with the same masks: loss {r_l:.4f}, gradients {r_g:.4f} ({n_g})")
    assert max(r_l, r_g) <= 1.0, (kind, r_l, (r_g, n_g))
    assert not torch.equal(loss, plain[0])
    # unpinned: the seed is drawn AFTER the step's own draws (they stay the p = 0 module's) and the generator ends one draw further
    free = step(m, kind, monkeypatch, pin=False)
    assert all((free[2].get(k) is None and plain[2].get(k) is None) or torch.equal(free[2][k], plain[2][k])
               for k in ("x_noise", "sigma", "labels", "noise", "cond", "dx", "x"))
    torch.manual_seed(1234)
    m0.training_step(batch(kind), 0)
    drawn = int(torch.randint(0, 2 ** 62, (1,)).item())
    assert torch.equal(free[3], torch.rand(1)) and int(m.model._drop_seed.item()) == drawn
    assert not torch.equal(free[0], loss)                                 # another seed, another loss
    # same seed, second step: the same bits
    again = step(m, kind, monkeypatch)
    assert torch.equal(again[0], loss) and all(torch.equal(again[1][n], grads[n]) for n in grads)
    # ---- eval(): the dropout = 0 module, bit for bit
    m.eval()
    ev = step(m, kind, monkeypatch, pin=False)
    assert torch.equal(ev[0], plain[0]) and all(torch.equal(ev[1][n], plain[1][n]) for n in grads)
    assert torch.equal(ev[3], plain[3])                                   # and no seed was drawn
    m.train()
    back = step(m, kind, monkeypatch)
    assert torch.equal(back[0], loss) and all(torch.equal(back[1][n], grads[n]) for n in grads)


@pytest.mark.parametrize("kind", KINDS)
def test_samplers_never_drop(kind):
    """sample_edm (and PlCondDdim.sample) of a dropout module in train() mode, right after a dropout training step, against the
    dropout = 0 module with the same weights: bit-identical."""
    m0, _ = make(kind, 0.0)
    m, _ = make(kind, P)
    m.training_step(batch(kind), 0).backward()                            # the plan now carries p > 0
    assert m.model.plan.dropout == P
    outs = []
    for mod in (m0, m):
        torch.manual_seed(99)
        if kind == "mcedm":
            cond, mk, _, _ = fx.sampler_inputs("det_u", 2, 32, 32)
            sp = hparams(fx.CFG_P, timesteps=3).sampler
            outs.append([mod.sample_edm(torch.zeros(2, 2, 32, 32).cuda(), cond.cuda(), mk.cuda(), sp, return_last=True)])
        else:
            h, u_noise, _ = fx.cond_sampler_inputs("det", 2, 32, 32)
            sp = (cond_hparams(timesteps=3) if kind == "cond_edm" else ddim_hparams()).sampler
            sp.timesteps = 3
            if kind == "cond_ddim_dx":
                mod.set_test_sampler_params(sp)
            res = [mod.sample_edm(h.cuda(), u_noise.cuda(), sp, return_last=True)]
            if kind == "cond_ddim_dx":
                from tests.test_cond_ddim_sample_cpu import sparams
                res.append(mod.sample(h.cuda(), u_noise.cuda(), sparams(timesteps=3), return_last=True))
            outs.append(res)
    for a, b in zip(*outs):
        a, b = (a[0] if isinstance(a, tuple) else a), (b[0] if isinstance(b, tuple) else b)
        assert torch.equal(a, b) and bool(torch.isfinite(a).all())


def test_flat_trainer_equals_the_module_path(monkeypatch):
    """EdmTrainer.step on a dropout module: loss and gradients equal PlMcedm.training_step's bit for bit at the same seed (the step
    replays from a HIP graph: the seed is read from device memory at replay); in eval() mode it is the p = 0 step."""
    from mcedm_amd.train import EdmTrainer, FlatTrainState
    m, _ = make("mcedm", P)
    m0, _ = make("mcedm", 0.0)
    h, u, mask, cond_noise, noise, rnd_normal = fx.training_inputs()
    xc, cond_in, mc = (t.cuda() for t in fx.training_nchw(h, u, mask, cond_noise))
    like = [cond_noise.cuda(), noise.cuda()]

    def module_step(mod):
        mod.zero_grad()
        q = list(like)
        with captured(monkeypatch), monkeypatch.context() as mp:
            mp.setattr(torch, "randn_like", lambda t, **k: q.pop(0))
            mp.setattr(torch, "randn", lambda *a, **k: rnd_normal)
            loss = mod.training_step(batch("mcedm"), 0)
        loss.backward()
        return loss.detach().clone(), torch.cat([p.grad.reshape(-1) for p in mod.model.parameters()]).clone()

    want, want0 = module_step(m), module_step(m0)
    assert not torch.equal(want[0], want0[0])
    monkeypatch.setattr(FlatTrainState, "_draw_seed", staticmethod(lambda: SEED))
    for mod, ref in ((m, want), (m0, want0)):
        tr = EdmTrainer(mod, lr=0.0)
        assert tr.dropout == mod.model.dropout
        for _ in range(2):                                                # the capture, then a replay
            loss = tr.step(xc, cond_in, mc, noise.cuda(), rnd_normal.cuda())
            assert torch.equal(loss.reshape(()), ref[0]) and torch.equal(tr.flat_g, ref[1])
    m.eval()
    tr = EdmTrainer(m, lr=0.0)
    loss = tr.step(xc, cond_in, mc, noise.cuda(), rnd_normal.cuda())
    assert torch.equal(loss.reshape(()), want0[0]) and torch.equal(tr.flat_g, want0[1])
