"""Golden vectors for dropout in the ADM U-Net (models/adm_blocks.py:170: conv1(dropout(x, p, training))), made by RUNNING THE
REFERENCE's ``DhariwalUNet`` on the CPU in ``train()`` mode with dropout = tests/_adm_dropout.py P_DROP on the rows GOLDEN_ROWS of
tests/_adm_arch.py.  ``torch.nn.functional.dropout`` is patched for the run so that the k-th call of a forward (= block k, the order
the network runs its blocks) applies the mask of mcedm_unet_plan_set_dropout's contract -- keep iff u >= p, kept values times
1 / (1 - p) -- with u from the NumPy restatement of the device generator at the recorded seed.  Stored per row: the network output F
of the training step, the loss, the squared norm of every parameter gradient (fp64 sums), three full gradients (conv_in.weight,
one encoder and one decoder conv1.weight), and F of the same network in ``eval()`` mode, which the script asserts to equal the
dropout = 0 network's bit for bit.

Only numbers and tags are stored (tests/golden/adm_dropout.npz): parameters, inputs and masks are regenerated from seeds and tags.

    python tools/make_golden_adm_dropout.py      # rewrites tests/golden/adm_dropout.npz (needs the reference checkout)
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import make_golden as mg            # noqa: E402  sets up the reference import and the Lightning stand-in

import torch                        # noqa: E402

from tests import _adm_arch as A   # noqa: E402
from tests import _adm_dropout as D   # noqa: E402


class ContractDropout:
    """Stands in for torch.nn.functional.dropout during one forward: call k applies masks[k]."""

    def __init__(self, masks, p):
        self.masks, self.p, self.k = list(masks), p, 0

    def __call__(self, x, p=0.5, training=True, inplace=False):
        assert abs(p - self.p) < 1e-12, (p, self.p)
        if not training:
            return x
        m = self.masks[self.k]
        self.k += 1
        assert tuple(m.shape) == tuple(x.shape), (self.k, tuple(m.shape), tuple(x.shape))
        return x * (m.to(x.dtype) * D.scale_of(self.p, x.dtype))


def build(tag, p):
    net = mg.build_reference(A.cfg_of(tag), A.SEED).model
    blocks = [b for b in net.modules() if isinstance(b, mg.ref_blocks.UNetBlock)]
    for b in blocks:
        b.dropout = p
    return net, len(blocks)


def main():
    torch.set_num_threads(A.CPU_THREADS)
    p = D.P_DROP
    out = {}
    F_nn = torch.nn.functional
    for tag in D.GOLDEN_ROWS:
        cfg, B, H, W = A.ARCHS[tag]
        masks = D.masks_for(cfg, B, H, W, p, D.SEED)
        net, nblocks = build(tag, p)
        assert nblocks == len(masks)
        P = A.params(tag)
        # eval(): no dropout, whatever p is -- bit for bit the dropout = 0 network
        net.eval()
        F_eval = D.training_F(tag, P, net=lambda x, labels, cond: net(x, labels, cond))
        with torch.no_grad():
            assert torch.equal(F_eval, D.training_F(tag, P)), f"{tag}: eval() mode is not the dropout = 0 network"
        # train(): the contract's masks in place of torch's own draws
        net.train()
        drop = ContractDropout(masks.values(), p)
        plain = F_nn.dropout
        F_nn.dropout = drop
        try:
            with torch.no_grad():
                F = D.training_F(tag, P, net=lambda x, labels, cond: net(x, labels, cond))
            assert drop.k == nblocks
            drop.k = 0
            net.zero_grad()
            loss = A.training_ref(tag, P, net=lambda x, labels, cond: net(x, labels, cond))
            loss.backward()
            assert drop.k == nblocks
        finally:
            F_nn.dropout = plain
        ref = {n: q.grad.detach().clone() for n, q in net.named_parameters()}
        assert A.bar_ratio(F, F_eval.detach()) > 100.0, f"{tag}: dropout must matter"
        # the fp32 oracle with the masks injected is the reference to rounding; the fp64 one shows the reference's own error
        loss64, g64 = D.training_grads(tag, masks, p)
        F64 = D.forward_F(tag, masks, p)
        r_grad, r_name = max((A.bar_ratio(ref[n], g64[n]), n) for n in ref)
        print(f"  {tag:7s} {len(ref):3d} parameters, {nblocks} blocks: reference fp32 vs the fp64 oracle with the same masks, worst err / bar: "
              f"forward {A.bar_ratio(F, F64):.4f}, loss {A.bar_ratio(loss.detach().reshape(1), loss64.reshape(1)):.4f}, "
              f"gradient {r_grad:.4f} ({r_name})", flush=True)
        out[f"{tag}::F"] = F
        out[f"{tag}::F_eval"] = F_eval.detach()
        out[f"{tag}::loss"] = loss.detach()
        out[f"{tag}::grad_sqnorm_each"] = torch.tensor([float((g.double() ** 2).sum()) for g in ref.values()], dtype=torch.float64)
        for n in D.golden_grad_names(tag):
            out[f"{tag}::grad::{n}"] = ref[n]
    mg.save("adm_dropout.npz", seed=D.SEED, p=p, cpu_threads=A.CPU_THREADS, **out)


if __name__ == "__main__":
    main()
