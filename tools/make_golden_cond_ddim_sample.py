"""Golden vectors for PlCondDdim.sample, the DDIM sampler of the single-task conditional DDPM on the ADM U-Net with
self-conditioning (models/ddim.py:1452-1530), made by RUNNING THE REFERENCE on the CPU with every random draw injected:

  * four sampling runs at B = 3, 32 x 32, return_last=False, both outputs (xs, x0_preds) stored whole -- CASES below;
  * validation_step and test_step (n_samples 2) with ``type: ddim`` at 4 steps: every logged metric and returned entry.

The parameters are those of tests/golden/cond_ddim.npz (tools/make_golden_cond_ddim.py: ``build`` / ``hparams``).

Injected draws.  ``torch.rand_like(x)`` of :1512 is a UNIFORM draw; step k (in the order the loop walks) gets the tagged uniform
``eta_draw(tag, k)`` = (fx.uniform(...) + 1) / 2 in [0, 1), fp32 -- a tagged uniform, not a mapped normal.  ``torch.randn_like`` of
the evaluation loops is injected as in oracle/make_golden_eval.py.

Before anything is written the script asserts that the final state of the plain run moves by at least 100 x the comparison
bar of tests/_tol.close_per_entry on at least half of its entries when (a) w goes 0 -> 0.5, (b) the self-conditioning feedback
is removed, (c) cond is zeroed: an implementation without the second pass, without the feedback or deaf to cond cannot pass.

    python tools/make_golden_cond_ddim_sample.py      # rewrites tests/golden/cond_ddim_sample.npz (needs the reference checkout)
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden_cond_ddim as G   # noqa: E402  sets up the reference import; build / hparams

import numpy as np                  # noqa: E402
import torch                        # noqa: E402

from oracle import fixtures as fx   # noqa: E402

mg = G.mg
B, H, W = G.B, G.H, G.W
# tag -> (timesteps, skip_type, eta, w)
CASES = {"uni": (10, "uniform", 0.0, 0.0), "cfg_eta": (10, "uniform", 0.5, 0.5), "quad": (8, "quad", 0.0, 0.0),
         "uneven": (7, "uniform", 0.0, 0.0)}
EVAL_STEPS, EVAL_N = 4, 2


def sampler(timesteps, skip_type="uniform", eta=0.0, w=0.0, **over):
    return mg.sampler_dict(name="ddim", type="ddim", timesteps=timesteps, skip_type=skip_type, eta=eta, w=w, **over)


def inputs():
    """Shared with tests/test_hip_cond_ddim_sample.py (same tags)."""
    return fx.randn("cddim/ddim/h", B, H, W, 1), fx.randn("cddim/ddim/u_noise", B, H, W, 1)


def eta_draw(tag, k):
    return torch.from_numpy(((fx.uniform(f"cddim/ddim/{tag}/eta{k}", B, 1, H, W) + 1.0) * 0.5).astype(np.float32))


class _Uniform:
    """torch.rand_like replaced by a queue of injected tensors."""

    def __init__(self, queue):
        self.queue = list(queue)

    def __enter__(self):
        self._rl = torch.rand_like

        def rand_like(t, **k):
            v = self.queue.pop(0)
            assert tuple(v.shape) == tuple(t.shape), (v.shape, t.shape)
            return v.to(t.dtype)
        torch.rand_like = rand_like
        return self

    def __exit__(self, *a):
        torch.rand_like = self._rl


def run(tag, timesteps, skip_type, eta, w, zero_cond=False, no_feedback=False):
    sp = sampler(timesteps, skip_type, eta, w)
    m = G.build(sp)
    h, un = inputs()
    if zero_cond:
        h = h * 0
    if no_feedback:
        net, fwd = m.ema_model.ma_model, m.ema_model.ma_model.forward
        net.forward = lambda x, t, cond=None, x_self_cond=None, dx=None: fwd(x, t, cond=cond, x_self_cond=None, dx=dx)
    with torch.no_grad(), _Uniform([eta_draw(tag, k) for k in range(2 * timesteps)]) as inj:
        xs, x0 = m.sample(h, un, mg._wrap(sp), return_last=False)
        used = 2 * timesteps - len(inj.queue)
    with torch.no_grad(), _Uniform([eta_draw(tag, k) for k in range(2 * timesteps)]):
        xs_last, x0_last = m.sample(h, un, mg._wrap(sp), return_last=True)
    assert torch.equal(xs_last[:, 0], xs[:, -1]) and torch.equal(x0_last[:, 0], x0[:, -1])
    assert xs.dtype == x0.dtype == torch.float32 and xs.shape[1] == x0.shape[1] + 1 and torch.isfinite(xs).all()
    assert used == (x0.shape[1] if abs(eta) > 1e-10 else 0)
    return xs, x0


def bars_apart(a, b):
    """|a - b| in units of close_per_entry's bar for reference b (rtol 1e-4, atol 1e-5 max|b|), per entry."""
    a, b = a.double(), b.double()
    return (a - b).abs() / (1e-5 * float(b.abs().max()) + 1e-4 * b.abs())


def record(module, logs):
    module.log = lambda name, value, **k: logs.__setitem__(name, torch.as_tensor(value).detach().clone())


def eval_module(sp, logs):
    m = G.build(sp)
    st = fx.STEP_NORM_STATS
    m.normalizer_input.set_stats(torch.tensor(st[0]), torch.tensor(st[1]))
    m.normalizer_target.set_stats(torch.tensor(st[2]), torch.tensor(st[3]))
    m.set_pde_loss_function("swe_per", False)
    m.current_epoch = 0
    record(m, logs)
    return m


def eval_inputs(which, n):
    """Shared with the test: un-normalised h, u 'b t x 1' and the injected randn_like '(n b) t x 1'."""
    st = fx.STEP_NORM_STATS
    h = fx.randn(f"cddim/ddim/{which}/h", fx.EVAL_B, H, W, 1) * st[1] + st[0]
    u = fx.randn(f"cddim/ddim/{which}/u", fx.EVAL_B, H, W, 1) * st[3] + st[2]
    return h, u, fx.randn(f"cddim/ddim/{which}/init", n * fx.EVAL_B, H, W, 1)


def main():
    out = {}
    for tag, (N, skip, eta, w) in CASES.items():
        xs, x0 = run(tag, N, skip, eta, w)
        out[f"{tag}::xs"], out[f"{tag}::x0_preds"] = xs, x0
        print(f"  {tag}: xs {tuple(xs.shape)} x0_preds {tuple(x0.shape)} max|x_last| {float(xs[:, -1].abs().max()):.3e}")
    assert out["uneven::x0_preds"].shape[1] == 8 and out["quad::x0_preds"].shape[1] == 8 and out["uni::x0_preds"].shape[1] == 10
    base = out["uni::xs"][:, -1]
    N, skip, eta, w = CASES["uni"]
    for what, kw in (("w 0 -> 0.5", dict(w=0.5)), ("no self-conditioning feedback", dict(w=w, no_feedback=True)),
                     ("cond zeroed", dict(w=w, zero_cond=True))):
        kw.setdefault("w", w)
        other = run("uni", N, skip, eta, **kw)[0][:, -1]
        share = float((bars_apart(other, base) >= 100.0).double().mean())
        print(f"  separation, {what}: {share:.3f} of the final state's entries move by >= 100 x the bar")
        assert share >= 0.5, (what, share)

    sp = sampler(EVAL_STEPS)
    logs = {}
    m = eval_module(sp, logs)
    h, u, init = eval_inputs("val", 1)
    with torch.no_grad(), mg._Inject([init]) as inj:
        res = m.validation_step((h, None, None, u), 0)
    assert not inj.like_queue and res.pop("epoch") == 0
    out.update({f"val::{k}": v for k, v in res.items()})
    out.update({f"val::log::{k}": v for k, v in logs.items()})

    sp = sampler(EVAL_STEPS, n_samples=EVAL_N)
    logs = {}
    m = eval_module(sp, logs)
    m.set_test_sampler_params(mg._wrap(sp))
    h, u, init = eval_inputs("test", EVAL_N)
    with torch.no_grad(), mg._Inject([init]) as inj:
        res = m.test_step((h, None, None, u), 0)
    assert not inj.like_queue
    out.update({f"test::{k}": v for k, v in res.items()})
    out.update({f"test::log::{k}": v for k, v in logs.items()})
    for k, v in out.items():
        if "::log::" in k:
            print(f"  {k} = {float(v):.6g}")
    mg.save("cond_ddim_sample.npz", seed=G.SEED, **out)


if __name__ == "__main__":
    main()
