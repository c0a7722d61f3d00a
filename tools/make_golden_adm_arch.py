"""Golden vectors for the ADM U-Net ``DhariwalUNet`` (models/adm_blocks.py:203-404) on every architecture of tests/_adm_arch.py,
made by RUNNING THE REFERENCE on the CPU: for each row the network's forward F at one noise level per sample, at one broadcast
label and -- where the row has conditioning channels -- with cond None, and the training step of tests/_adm_arch.py
training_ref through the reference network's own autograd: the loss, the squared norm of every parameter gradient (fp64 sums)
and the full gradients of three small tensors.

Before anything is written the script asserts, for every row, that ``named_parameters()`` equals mcedm_oracle.param_shapes in
order and that the oracle's fp32 forward equals the reference's bit for bit, and it prints how far the reference's own fp32
numbers lie from the fp64 evaluation of the same formula, in units of the comparison bar (rtol 1e-4, atol 1e-5 max|ref|).
Only outputs are stored (tests/golden/adm_arch.npz): parameters and inputs are regenerated from seeds and tags.

    python tools/make_golden_adm_arch.py      # rewrites tests/golden/adm_arch.npz (needs the reference checkout)
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import make_golden as mg            # noqa: E402  sets up the reference import and the Lightning stand-in

import torch                        # noqa: E402

from tests import _adm_arch as A   # noqa: E402


def build(tag):
    cfg = A.cfg_of(tag)
    net = mg.build_reference(cfg, A.SEED).model.eval()
    named = [(n, tuple(p.shape)) for n, p in net.named_parameters()]
    assert named == [(n, tuple(s)) for n, s in A.orc.param_shapes(cfg)], f"{tag}: param_shapes drifted from the reference DhariwalUNet"
    return net


def main():
    torch.set_num_threads(A.CPU_THREADS)
    out = {}
    for tag in A.ARCHS:
        net = build(tag)
        P = A.params(tag)
        P64 = A.params(tag, torch.float64)
        worst = 0.0
        for key, kind in A.runs(tag):
            _, F = A.denoise_ref(tag, P, kind, net=net)
            assert F.dtype == torch.float32 and torch.isfinite(F).all()
            assert torch.equal(A.denoise_ref(tag, P, kind)[1], F), f"{key}: the fp32 oracle is not the reference bit for bit"
            worst = max(worst, A.bar_ratio(F, A.denoise_ref(tag, P64, kind)[1]))
            out[key] = F
        if A.cfg_of(tag).cond_channels:                            # cond must matter
            assert A.bar_ratio(out[f"{tag}::F_label"], out[f"{tag}::F_nocond"]) > 100.0, tag
        # the training step through the reference network's autograd
        net.zero_grad()
        loss = A.training_ref(tag, P, net=net)
        loss.backward()
        ref = {n: p.grad.detach().clone() for n, p in net.named_parameters()}
        loss64, g64 = A.training_grads(tag)
        r_loss = A.bar_ratio(loss.detach().reshape(1), loss64.reshape(1))
        r_grad, r_name = max((A.bar_ratio(ref[n], g64[n]), n) for n in ref)
        out[f"{tag}::loss"] = loss.detach()
        out[f"{tag}::grad_sqnorm_each"] = torch.tensor([float((g.double() ** 2).sum()) for g in ref.values()], dtype=torch.float64)
        for n in A.grad_names(tag):
            out[f"{tag}::grad::{n}"] = ref[n]
        print(f"  {tag:7s} {len(ref):3d} parameters, max|F| {float(F.abs().max()):.3f}: reference fp32 vs the fp64 formula, worst err / bar: "
              f"forward {worst:.4f}, loss {r_loss:.4f}, gradient {r_grad:.4f} ({r_name})", flush=True)
    mg.save("adm_arch.npz", seed=A.SEED, **out)


if __name__ == "__main__":
    main()
