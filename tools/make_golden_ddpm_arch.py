"""Golden vectors for the DDPM U-Net ``Model`` (models/ddim_blocks.py:222-470) on every architecture of tests/_ddpm_arch.py, made by
RUNNING THE REFERENCE on the CPU: for each row ``Model(x, t, cond, x_self_cond)`` at t = 3 and t = 937 -- a plain network with
x_self_cond given and None, a network with the cond_enc / combine_enc head or with cat_cond with cond given and None.

Before anything is written the script asserts, for every row, that ``named_parameters()`` equals ddpm_oracle.param_shapes in
order and that the oracle's fp32 forward equals the reference's bit for bit, and it prints how far the reference's own fp32
output lies from the fp64 evaluation of the same formula, in units of the comparison bar (rtol 1e-4, atol 1e-5 max|ref|).
Only the outputs are stored (tests/golden/ddpm_arch.npz, a few hundred kB): parameters and inputs are regenerated from seeds
and tags.

    python tools/make_golden_ddpm_arch.py      # rewrites tests/golden/ddpm_arch.npz (needs the reference checkout)
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import make_golden as mg            # noqa: E402  sets up the reference import and the Lightning stand-in

import torch                        # noqa: E402
from models.ddim_blocks import Model  # noqa: E402  (reference)

from tests import _ddpm_arch as A   # noqa: E402


def hparams(cfg):
    """The fields Model.__init__ reads (configs/model/ddim_res32.yaml, ddim_cond_h_res32.yaml, edm_cond_h_res32.yaml)."""
    return mg._wrap(dict(
        model=dict(type="simple", in_channels=cfg.in_channels, cond_channels=cfg.cond_channels, cat_cond=cfg.cat_cond, out_ch=cfg.out_ch,
                   ch=cfg.ch, ch_mult=list(cfg.ch_mult), num_res_blocks=cfg.num_res_blocks, attn_resolutions=list(cfg.attn_resolutions),
                   dropout=0.0, resamp_with_conv=True, resolution=cfg.resolution, self_cond=cfg.self_cond, dx_cond=False, cat_dx=False),
        diffusion=dict(num_diffusion_timesteps=cfg.num_timesteps)))


def build(tag):
    cfg = A.ALL[tag]
    net = Model(hparams(cfg)).eval()
    named = [(n, tuple(p.shape)) for n, p in net.named_parameters()]
    assert named == [(n, tuple(s)) for n, s in A.ddo.param_shapes(cfg)], f"{tag}: param_shapes drifted from the reference Model"
    P = A.params(tag)
    with torch.no_grad():
        for n, p in net.named_parameters():
            p.copy_(P[n])
    return net, P


def main():
    torch.set_num_threads(A.CPU_THREADS)
    out = {}
    for tag in A.ALL:
        net, P = build(tag)
        P64 = A.params(tag, torch.float64)
        x, xsc, cond = A.inputs(tag)
        worst = 0.0
        for run in A.runs(tag):
            key, t, use_sc, use_cond = run
            with torch.no_grad():
                y = net(x, torch.full((A.B,), t), cond=cond if use_cond else None, x_self_cond=xsc if use_sc else None)
            assert y.dtype == torch.float32 and torch.isfinite(y).all()
            assert torch.equal(A.oracle_forward(tag, P, run), y), f"{key}: the fp32 oracle is not the reference bit for bit"
            worst = max(worst, A.bar_ratio(y, A.oracle_forward(tag, P64, run)))
            out[key] = y
        a, b = (out[r[0]] for r in A.runs(tag)[:2])              # x_self_cond / cond must matter
        assert A.bar_ratio(a, b) > 100.0, tag
        print(f"  {tag:14s} {len(A.runs(tag))} runs, max|ref| {float(y.abs().max()):.3f}: reference fp32 vs fp64 formula, worst err / bar {worst:.4f}")
    mg.save("ddpm_arch.npz", seed=A.SEED, **out)


if __name__ == "__main__":
    main()
