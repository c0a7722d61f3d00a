"""What the CPU and the GPU tests of the kernels that close a training step share (csrc/edm.hip: noise inputs, the two losses,
the squared gradient norm, clip + Adam + EMA): the hyper-parameter table, the seeded inputs, the fp64 references and the fp32
yardstick.  torch only: nothing here loads the GPU library.

The yardstick.  The Adam kernel works in fp32, so it cannot agree with fp64 better than fp32 arithmetic allows, and how well
that is depends on the hyper-parameters, the step count and the data.  Instead of a guessed tolerance the tests measure it:
``torch.optim.Adam`` (+ ``clip_grad_norm_`` + the EMA formula) runs on fp32 CPU tensors with the SAME inputs, and
``e32 = max|fp32 - fp64|`` per tensor is what a correct fp32 implementation loses.  The kernel is held to ``FACTOR x e32``; the
factor allows for the device's sqrtf / division and the clip factor (formed in fp64 on the device, in fp32 by torch), which
differ from the CPU's by an ulp per operation.  ``e32`` never comes from the kernel's output.
"""
import math
from collections import namedtuple

import torch

FACTOR = 4.0
U = 2.0 ** -24                         # unit roundoff of fp32: one rounding loses at most U x |value|
N_ADAM = 70001                         # 274 blocks, no multiple of 256
STEPS = 12

# max_norm None: no clipping (the kernel gets no squared norm); ema_beta None: no EMA buffer
Row = namedtuple("Row", "name lr b1 b2 eps wd max_norm grad_scale ema_beta")
ROWS = [
    Row("A", 2e-4, 0.9, 0.999, 1e-8, 0.0, 1.0, 1.0, 0.999),        # the reference's configuration, clip active
    Row("B", 1e-2, 0.8, 0.95, 1e-3, 1e-2, 1.0, 0.5, 0.99),         # every hyper-parameter away from its default
    Row("C", 1e-2, 0.5, 0.9, 1e-8, 0.0, None, 1.0, None),          # no clip, no EMA
    Row("D", 1e-2, 0.9, 0.999, 1e-8, 1e-2, 1e3, 1.0, 0.999),       # clip computed but inactive
    Row("E", 1e-2, 0.0, 0.999, 1e-8, 0.0, 1.0, 1.0, 0.9),          # beta1 = 0: exp_avg is the gradient
]
ROW = {r.name: r for r in ROWS}


def gen(seed):
    return torch.Generator().manual_seed(seed)


def grad_sequence(n, steps, seed=1234):
    """``steps`` fp32 gradients of n elements.  The scale alternates between 3.0 and 0.05 from step to step (the clip factor
    changes every step -- for small n the clip switches on and off -- and exp_avg_sq remembers the large step during the small
    one); every 7th element is exactly 0 (sqrt(0) / bc + eps, and with weight decay a gradient that is the decay alone)."""
    g = gen(seed)
    out = []
    for k in range(steps):
        t = torch.randn(n, generator=g, dtype=torch.float32) * (3.0 if k % 2 == 0 else 0.05)
        t[::7] = 0.0
        out.append(t)
    return out


def params(n, seed=99):
    """(p0, ema0): the EMA copy starts away from the parameters, as after some training."""
    g = gen(seed)
    p0 = torch.randn(n, generator=g, dtype=torch.float32)
    return p0, p0 + 0.01 * torch.randn(n, generator=g, dtype=torch.float32)


def moments(n, seed=7):
    """Non-zero (exp_avg, exp_avg_sq >= 0) for a run that starts late.  Every 11th element has seen zero gradients only: both
    moments are exactly 0 there (with a zero gradient the update is 0 / (0 + eps))."""
    g = gen(seed)
    m0 = 0.1 * torch.randn(n, generator=g, dtype=torch.float32)
    v0 = 0.01 * torch.rand(n, generator=g, dtype=torch.float32)
    m0[::11] = 0.0
    v0[::11] = 0.0
    return m0, v0


# ---------------------------------------------------------------------------------------------- clip + Adam + EMA, fp64
def adam_ema_ref(p, g, m, v, ema, step, lr, b1, b2, eps, wd, sqnorm, max_norm, grad_scale, ema_beta):
    """One step in fp64, nothing modified in place; returns (p, m, v, ema).  ``sqnorm``: the squared norm of the UNSCALED
    gradient, or None for no clipping.  clip_grad_norm_ on the scaled gradient, then torch.optim.Adam (no amsgrad: weight decay
    joins the clipped gradient), then EmaModel.update_average (old * beta + (1 - beta) * new)."""
    p, g, m, v = (torch.as_tensor(t).double() for t in (p, g, m, v))
    clip = 1.0
    if sqnorm is not None:
        total = math.sqrt(float(sqnorm)) * grad_scale
        clip = min(1.0, max_norm / (total + 1e-6))
    g = g * grad_scale * clip + wd * p
    m = m + (g - m) * (1.0 - b1)
    v = v * b2 + (1.0 - b2) * g * g
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    p = p - (lr / bc1) * (m / (v.sqrt() / math.sqrt(bc2) + eps))
    if ema is not None:
        ema = torch.as_tensor(ema).double() * ema_beta + (1.0 - ema_beta) * p
    return p, m, v, ema


Run = namedtuple("Run", "p_steps m v ema")      # p after every step; the other three after the last


def ref_run(row, p0, ema0, grads, m0=None, v0=None, step0=0, lr_at=None):
    """adam_ema_ref over ``grads`` (flat tensors) from (p0, m0 or 0, v0 or 0, ema0) with steps step0 + 1, ...;
    ``lr_at(k)``: the learning rate of the k-th call (0-based), default row.lr."""
    p, ema = p0.double(), None if row.ema_beta is None else ema0.double()
    m = torch.zeros_like(p) if m0 is None else m0.double()
    v = torch.zeros_like(p) if v0 is None else v0.double()
    ps = []
    for k, g in enumerate(grads):
        sq = None if row.max_norm is None else float((g.double() ** 2).sum())
        p, m, v, ema = adam_ema_ref(p, g, m, v, ema, step0 + k + 1, row.lr if lr_at is None else lr_at(k), row.b1, row.b2, row.eps,
                                    row.wd, sq, row.max_norm, row.grad_scale, row.ema_beta)
        ps.append(p)
    return Run(ps, m, v, ema)


def torch_run(row, dtype, p0s, ema0s, grads, m0s=None, v0s=None, step0=0, lr_at=None):
    """torch.optim.Adam + clip_grad_norm_ + the EMA formula on CPU tensors of ``dtype``.  p0s / ema0s / m0s / v0s: lists of tensors
    (one per parameter), grads: per step a list of tensors.  grad_scale is folded in by scaling .grad.  Returns a Run of flat
    (concatenated) tensors."""
    ps = [torch.nn.Parameter(t.detach().clone().to(dtype)) for t in p0s]
    emas = None if row.ema_beta is None else [t.detach().clone().to(dtype) for t in ema0s]
    opt = torch.optim.Adam(ps, lr=row.lr, betas=(row.b1, row.b2), eps=row.eps, weight_decay=row.wd, foreach=False)
    if m0s is not None:
        for p, m, v in zip(ps, m0s, v0s):
            opt.state[p] = {"step": torch.tensor(float(step0)), "exp_avg": m.detach().clone().to(dtype),
                            "exp_avg_sq": v.detach().clone().to(dtype)}
    flat = lambda ts: torch.cat([t.detach().flatten() for t in ts]).clone()      # noqa: E731
    p_steps = []
    for k, gs in enumerate(grads):
        if lr_at is not None:
            opt.param_groups[0]["lr"] = lr_at(k)
        for p, g in zip(ps, gs):
            p.grad = g.detach().clone().to(dtype) * row.grad_scale
        if row.max_norm is not None:
            torch.nn.utils.clip_grad_norm_(ps, row.max_norm)
        opt.step()
        if emas is not None:
            with torch.no_grad():
                emas = [e * row.ema_beta + (1 - row.ema_beta) * p for e, p in zip(emas, ps)]
        p_steps.append(flat(ps))
    return Run(p_steps, flat([opt.state[p]["exp_avg"] for p in ps]), flat([opt.state[p]["exp_avg_sq"] for p in ps]),
               None if emas is None else flat(emas))


Yard = namedtuple("Yard", "ref e32_p e32_m e32_v e32_ema movement")


def yardstick(row, p0, ema0, grads, m0=None, v0=None, step0=0, lr_at=None):
    """The fp64 reference of a flat run and what torch's own fp32 Adam loses against it on the same inputs: ``e32_p[k]`` after
    step k, the other three after the last step; ``movement``: max|p_fp64 - p0| after the last step."""
    ref = ref_run(row, p0, ema0, grads, m0, v0, step0, lr_at)
    wrap = lambda t: None if t is None else [t]                                   # noqa: E731
    f32 = torch_run(row, torch.float32, [p0], wrap(ema0), [[g] for g in grads], wrap(m0), wrap(v0), step0, lr_at)
    return against(ref, f32, p0)


def against(ref, f32, p0):
    err = lambda a, b: None if b is None else float((a.double() - b.double()).abs().max())      # noqa: E731
    return Yard(ref, [err(a, b) for a, b in zip(f32.p_steps, ref.p_steps)], err(f32.m, ref.m), err(f32.v, ref.v), err(f32.ema, ref.ema),
                float((ref.p_steps[-1] - p0.double()).abs().max()))


# ---------------------------------------------------------------------------------------------- losses, fp64
def edm_weight(sigma, sigma_data):
    s = torch.as_tensor(sigma).double()
    return (s * s + sigma_data ** 2) / (s * sigma_data) ** 2


def edm_loss_ref(D, x, mask, sigma, sigma_data):
    """mean_b sum_chw w_b (D m - x m)^2 and its gradient (2 w_b / B) (D m - x m) m, in fp64; ``mask`` None: m = 1."""
    D, x = D.double(), x.double()
    m = torch.ones_like(D) if mask is None else mask.double()
    w = edm_weight(sigma, sigma_data).view(-1, 1, 1, 1)
    diff = D * m - x * m
    return (w * diff * diff).sum(dim=(1, 2, 3)).mean(), (2.0 * w / D.shape[0]) * diff * m


def eps_loss_ref(F, eps):
    """mean_b sum_chw (F - eps)^2 and its gradient (2 / B) (F - eps), in fp64."""
    diff = F.double() - eps.double()
    return (diff * diff).sum(dim=(1, 2, 3)).mean(), (2.0 / F.shape[0]) * diff


# two sweeps of 64 blocks / per_sample < 256 / B > 64 / B > 64 with enough elements for 64 blocks, so the table's RED_MAX / B = 63
# caps the grid / one block per sample, every slot of the table in use
LOSS_SHAPES = [(1, 2, 128, 128), (3, 2, 5, 7), (65, 2, 16, 16), (65, 1, 127, 127), (4096, 1, 3, 3)]
RED_MAX = 4096                         # slots of the fixed-order reduction (csrc/edm.hip)


def loss_grid(shape):
    """(gx, k) of mcedm_edm_loss / mcedm_eps_loss: blocks per sample, and terms per thread."""
    B, C, H, W = shape
    per = C * H * W
    gx = min(64, -(-per // 256), RED_MAX // B)
    return gx, -(-per // (gx * 256))


def loss_sigmas(B):
    """The noise levels a loss case runs with: 0.002 to 80 over the batch (log-spaced); a batch of one runs both ends and 0.4."""
    if B == 1:
        return [torch.tensor([v], dtype=torch.float32) for v in (0.002, 0.4, 80.0)]
    return [torch.exp(torch.linspace(math.log(0.002), math.log(80.0), B)).float()]


def loss_inputs(shape, seed=5):
    """D (or F), x (or eps), a 0/1 mask, a non-binary mask."""
    g = gen(seed + shape[0])
    D = torch.randn(shape, generator=g)
    x = torch.randn(shape, generator=g)
    m01 = (torch.rand(shape, generator=g) < 0.6).float()
    mfrac = torch.rand(shape, generator=g) * 1.5
    return D, x, m01, mfrac


def sqnorm_terms(n):
    """Most fp32 terms one accumulator of sqnorm_kernel adds: ceil(n / 524288) elements per thread over two accumulators."""
    per_thread = -(-n // 524288)
    return -(-per_thread // 2)


def ddpm_tables(n=1000):
    """(sqrt(abar_t), sqrt(1 - abar_t)) of the linear beta schedule, fp32 as the modules hold them."""
    ab = torch.cumprod(1.0 - torch.linspace(1e-4, 2e-2, n, dtype=torch.float64), 0)
    return ab.sqrt().float(), (1.0 - ab).sqrt().float()
