"""CPU: the fp64 references of tests/_train_ops.py pinned against torch itself, and the conditions the GPU tests of the
training-step kernels (tests/test_hip_train_ops.py) rely on: that the multi-step cases see what a single step from zero moments
cannot, that the fp32 yardstick is small against the movement of the parameters, and that the case tables reach the grid caps
they are meant to reach."""
import math

import pytest
import torch

from tests import _train_ops as T


def close12(a, b, what=""):
    """rtol 1e-12 of the element, or of the tensor's largest element where an element is what a cancellation left (exp_avg sums
    terms of either sign, a parameter may cross zero): there the last bit of the clip factor, which torch forms from per-tensor
    norms, is all that remains of it."""
    torch.testing.assert_close(a, b, rtol=1e-12, atol=1e-12 * float(b.abs().max()), msg=lambda s: f"{what}: {s}")


def flat_inputs(n=T.N_ADAM, steps=T.STEPS):
    p0, ema0 = T.params(n)
    return p0, ema0, T.grad_sequence(n, steps)


@pytest.fixture(scope="module")
def inputs():
    return flat_inputs()


@pytest.mark.parametrize("row", T.ROWS, ids=lambda r: r.name)
def test_adam_ema_ref_equals_torch_adam_in_fp64(inputs, row):
    p0, ema0, grads = inputs
    ref = T.ref_run(row, p0, ema0, grads)
    # two parameters of unequal size: the clip uses the norm over both
    cut = T.N_ADAM // 3
    split = lambda t: [t[:cut], t[cut:]]                                          # noqa: E731
    tr = T.torch_run(row, torch.float64, split(p0), split(ema0), [split(g) for g in grads])
    for k in range(T.STEPS):
        close12(ref.p_steps[k], tr.p_steps[k], f"p after step {k + 1}")
    close12(ref.m, tr.m, "exp_avg")
    close12(ref.v, tr.v, "exp_avg_sq")
    if row.ema_beta is None:
        assert ref.ema is None and tr.ema is None
    else:
        close12(ref.ema, tr.ema, "ema")


def test_adam_ema_ref_from_given_moments_at_a_late_step():
    n, row, step = 4099, T.ROW["B"], 100000
    p0, ema0 = T.params(n)
    m0, v0 = T.moments(n)
    g = T.grad_sequence(n, 1)
    ref = T.ref_run(row, p0, ema0, g, m0, v0, step - 1)
    tr = T.torch_run(row, torch.float64, [p0], [ema0], [g], [m0], [v0], step - 1)
    for a, b in zip((ref.p_steps[0], ref.m, ref.v, ref.ema), (tr.p_steps[0], tr.m, tr.v, tr.ema)):
        close12(a, b)
    assert bool((v0 == 0).any()) and bool((v0 >= 0).all())


def test_one_step_from_zero_moments_cannot_see_the_betas(inputs):
    """p1 = p0 - lr * g / (|g| + eps) whatever beta1 and beta2 are: a test of step 1 alone passes with the betas swapped, with a
    wrong bias correction or a wrong lerp.  From step 2 on they show, far above the bound the GPU tests use."""
    p0, ema0, grads = inputs
    a = T.ROW["D"]
    b = a._replace(b1=a.b2, b2=a.b1)
    ya = T.yardstick(a, p0, ema0, grads)
    rb = T.ref_run(b, p0, ema0, grads)
    close12(ya.ref.p_steps[0], rb.p_steps[0], "p after step 1")
    for k in range(1, T.STEPS):
        gap = float((ya.ref.p_steps[k] - rb.p_steps[k]).abs().max())
        print(f"step {k + 1}: betas swapped move p by {gap:.3e}, bound {T.FACTOR * ya.e32_p[k]:.3e}")
        assert gap > 100 * T.FACTOR * ya.e32_p[k]


@pytest.mark.parametrize("row", T.ROWS, ids=lambda r: r.name)
def test_fp32_yardstick_is_small_against_the_movement(inputs, row):
    p0, ema0, grads = inputs
    y = T.yardstick(row, p0, ema0, grads)
    print(f"row {row.name}: e32 p {y.e32_p[-1]:.3e} m {y.e32_m:.3e} v {y.e32_v:.3e} ema {y.e32_ema} movement {y.movement:.3e}")
    assert all(0 < e < 1e-5 for e in y.e32_p) and 0 < y.e32_m and 0 < y.e32_v
    assert (y.e32_ema is None) == (row.ema_beta is None)
    if row.lr == 1e-2:                # a 1 % error in the update is 10 x FACTOR x e32 at the least
        assert y.movement >= 1000 * y.e32_p[-1]


def test_gradient_sequence():
    grads = T.grad_sequence(T.N_ADAM, T.STEPS)
    again = T.grad_sequence(T.N_ADAM, T.STEPS)
    assert all(torch.equal(a, b) for a, b in zip(grads, again))
    for k, g in enumerate(grads):
        assert g.dtype == torch.float32 and bool((g[::7] == 0).all()) and int((g == 0).sum()) == -(-T.N_ADAM // 7)
        assert abs(float(g.std()) / (3.0 if k % 2 == 0 else 0.05) - math.sqrt(6 / 7)) < 0.02
    norms = [float(g.double().norm()) for g in grads]
    # n = 70001: max_norm 1 clips at every step by a factor that alternates (rows A, E; B sees half the norm); 1e3 never does
    assert all(0.5 * v > 2.0 for v in norms) and max(norms) < 1e3 - 1
    # for the small sizes of the edge tests, and the toy module's 146 parameters, the clip switches on and off
    for n in (255, 146):
        small = [float(g.double().norm()) * 0.5 for g in T.grad_sequence(n, 4)]
        assert small[0] > 1 > small[1] and small[2] > 1 > small[3]


def test_loss_references_equal_autograd():
    shape = (3, 2, 5, 7)
    D, x, m01, mfrac = T.loss_inputs(shape)
    sigma, = T.loss_sigmas(shape[0])
    for mask in (m01, mfrac, None):
        for sd in (0.5, 1.0):
            Dg = D.double().requires_grad_(True)
            m = torch.ones_like(Dg) if mask is None else mask.double()
            s = sigma.double().view(-1, 1, 1, 1)
            w = (s ** 2 + sd ** 2) / (s * sd) ** 2                               # models/losses.py: the EDM weight
            (w * (Dg * m - x.double() * m) ** 2).sum(dim=(1, 2, 3)).mean().backward()
            loss, dD = T.edm_loss_ref(D, x, mask, sigma, sd)
            torch.testing.assert_close(loss, (w * (Dg.detach() * m - x.double() * m) ** 2).sum(dim=(1, 2, 3)).mean(), rtol=1e-13, atol=0)
            torch.testing.assert_close(dD, Dg.grad, rtol=1e-12, atol=1e-300)
    Fg = D.double().requires_grad_(True)
    ((Fg - x.double()) ** 2).sum(dim=(1, 2, 3)).mean().backward()
    loss, dF = T.eps_loss_ref(D, x)
    torch.testing.assert_close(loss, ((D.double() - x.double()) ** 2).sum(dim=(1, 2, 3)).mean(), rtol=1e-13, atol=0)
    torch.testing.assert_close(dF, Fg.grad, rtol=1e-12, atol=1e-300)


def test_case_tables_reach_the_grid_caps():
    assert [T.loss_grid(s) for s in T.LOSS_SHAPES] == [(64, 2), (1, 1), (2, 1), (63, 2), (1, 1)]
    assert T.LOSS_SHAPES[1][1] * T.LOSS_SHAPES[1][2] * T.LOSS_SHAPES[1][3] < 256
    assert [T.sqnorm_terms(n) for n in (0, 1, 255, 257, 524288, 524289, 1048577, 1572868)] == [0, 1, 1, 1, 1, 1, 2, 2]
    for shape in T.LOSS_SHAPES:
        D, x, m01, mfrac = T.loss_inputs(shape)
        assert set(m01.unique().tolist()) <= {0.0, 1.0} and 0 < float(m01.mean()) < 1 and float(mfrac.max()) > 1
        sigmas = torch.cat(T.loss_sigmas(shape[0]))
        assert sigmas.dtype == torch.float32 and sigmas.numel() == (3 if shape[0] == 1 else shape[0])
        assert abs(float(sigmas.min()) / 0.002 - 1) < 1e-6 and abs(float(sigmas.max()) / 80 - 1) < 1e-6
    a, b = T.ddpm_tables()
    assert a.dtype == torch.float32 and a.numel() == 1000 and float(a[999]) < 0.01 < float(a[0])
    torch.testing.assert_close(a.double() ** 2 + b.double() ** 2, torch.ones(1000, dtype=torch.float64), rtol=0, atol=1e-6)
