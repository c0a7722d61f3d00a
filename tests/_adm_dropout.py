"""What the dropout tests of the ADM U-Net and tools/make_golden_adm_dropout.py share: the mask contract of
mcedm_unet_plan_set_dropout restated on the host, and an fp64 (or fp32) oracle WITH dropout that needs no edit under oracle/.

The contract.  Block j is the 0-based position of a block in the order the network runs them (encoder, then decoder); with
u = draw j of the uniform generator (mcedm_uniform_fill; tests/test_hip_sampler_noise.py uniform_ref restates it in NumPy) over
conv1's input [B, cout, H, W] in memory order, an element is kept iff u >= float32(p) and a kept value is multiplied by
float32(1) / (float32(1) - float32(p)).

The oracle.  ``injected(P, masks, p)`` wraps ``oracle.mcedm_oracle.conv2d`` for the duration of a ``with`` block: a call whose
weight IS a block's ``conv1.weight`` in ``P`` (matched by identity) first multiplies its input by that block's mask times 1 / (1 - p),
in the tensor's dtype -- models/adm_blocks.py:170 ``conv1(dropout(x))``.  Everything else is the oracle as it stands, so autograd
through it gives the reference gradients.
"""
import contextlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import mcedm_oracle as orc  # noqa: E402
from tests import _adm_arch as A  # noqa: E402
from tests.test_hip_sampler_noise import uniform_ref  # noqa: E402  (the NumPy Philox restatement)

P_DROP = 0.25                             # of the network tests and of tests/golden/adm_dropout.npz
SEED = 0x2545F4914F6CDD1D                 # the recorded seed of the golden (any 62-bit value)
GOLDEN_ROWS = ("narrow", "rect")          # rows of tests/_adm_arch.py ARCHS the reference was run on
ROWS = ("narrow", "ragged", "rect", "c128a", "ch24")      # rows of the GPU training-step test


def block_shapes(cfg, B, H, W):
    """(key, [B, cout, H_j, W_j]) of every block's conv1 input, in execution order: the draw index is the position."""
    spec = orc.build_spec(cfg)
    out = []
    for b in spec.enc + spec.dec:
        res = int(b.key.split(".")[1].split("x")[0])
        level = (cfg.resolution // res).bit_length() - 1
        out.append((b.key, (B, b.cout, H >> level, W >> level)))
    return out


def keep_numpy(seed, draw, shape, p):
    """The contract's keep mask (float32 zeros and ones) from the NumPy generator."""
    u = uniform_ref(int(seed), int(draw), int(np.prod(shape)))
    return torch.from_numpy((u >= np.float32(p)).astype(np.float32).reshape(shape))


def keep_device(L, seed_t, draw, shape, p):
    """The same from mcedm_uniform_fill on the GPU (seed_t: int64 [1] on the device) -> a CPU tensor."""
    u = L.uniform_fill(torch.empty(shape, dtype=torch.float32, device=seed_t.device), seed_t, draw)
    return (u >= float(np.float32(p))).to(torch.float32).cpu()


def masks_for(cfg, B, H, W, p, seed, keep=None):
    """key -> keep mask of every block.  keep(draw, shape) overrides the NumPy generator (the GPU tests pass the device's)."""
    keep = keep or (lambda j, shape: keep_numpy(seed, j, shape, p))
    return {key: keep(j, shape) for j, (key, shape) in enumerate(block_shapes(cfg, B, H, W))}


def scale_of(p, dtype):
    """1 / (1 - p) of the contract's fp32 p, formed in ``dtype``."""
    one = torch.ones((), dtype=dtype)
    return one / (one - torch.tensor(float(np.float32(p)), dtype=dtype))


@contextlib.contextmanager
def injected(P, masks, p):
    """The oracle with dropout: see the module docstring.  Counts the injections: every block exactly once per forward."""
    by_id = {id(P[f"{k}.conv1.weight"]): k for k in masks}
    plain = orc.conv2d
    hits = []

    def conv2d(x, w, b, up=False, down=False):
        k = by_id.get(id(w)) if w is not None else None
        if k is not None and w is P[f"{k}.conv1.weight"]:
            m = masks[k]
            assert tuple(m.shape) == tuple(x.shape), (k, tuple(m.shape), tuple(x.shape))
            x = x * (m.to(x.dtype) * scale_of(p, x.dtype))
            hits.append(k)
        return plain(x, w, b, up=up, down=down)

    orc.conv2d = conv2d
    try:
        yield hits
    finally:
        orc.conv2d = plain


def training_grads(tag, masks, p=P_DROP, dtype=torch.float64):
    """(loss, name -> gradient) of tests/_adm_arch.py training_ref through the oracle with the masks injected."""
    P = {k: v.requires_grad_(True) for k, v in A.params(tag, dtype).items()}
    with injected(P, masks, p) as hits:
        loss = A.training_ref(tag, P)
    assert sorted(hits) == sorted(masks), (len(hits), len(masks))
    grads = torch.autograd.grad(loss, list(P.values()))
    return loss.detach(), dict(zip(P, grads))


def forward_F(tag, masks, p=P_DROP, dtype=torch.float64):
    """The network output F of the training step's forward (the 'sigma'-free part is enough to pin position and scale): the oracle
    on the training step's own inputs, masks injected."""
    P = A.params(tag, dtype)
    with torch.no_grad(), injected(P, masks, p):
        return training_F(tag, P)


def training_F(tag, P, net=None):
    """F of the training step of tests/_adm_arch.py training_ref (same inputs, same noise levels), without the loss around it."""
    dt = next(iter(P.values())).dtype
    f = A._network(P, tag, net)
    I = A.inputs(tag)
    x = I["x"].to(dt)
    cond = None if I["cond"] is None else I["cond"].to(dt)
    if tag in A.PLAIN:
        return f(x, A.plain_labels(tag).to(dt), cond)
    sigma = (I["rnd_normal"].double().to(dt) * orc.P_STD + orc.P_MEAN).exp()
    x_noise = x + I["mask"].to(dt) * I["noise"].to(dt) * sigma
    _, _, c_in, c_noise = orc.precond_coeffs(sigma)
    return f(c_in * x_noise, c_noise.flatten(), cond)


def golden_grad_names(tag):
    """The three full gradients the fixture stores per row: conv_in.weight, one encoder conv1.weight, one decoder conv1.weight
    (of each half the LAST block of the smallest width: the fixture stays small)."""
    spec = orc.build_spec(A.cfg_of(tag))
    pick = lambda blocks: min(reversed(blocks), key=lambda b: b.cout).key      # noqa: E731
    return [f"{spec.conv_in_key}.weight", f"{pick(spec.enc)}.conv1.weight", f"{pick(spec.dec)}.conv1.weight"]
