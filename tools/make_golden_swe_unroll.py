"""Golden vectors for the device-side SWE unroll (mcedm_swe_fv_unroll; SweFvLoss.unroll_from_init / unroll_loss and
PlCondEdm.print_unroll_metrics of the drop-ins), made by RUNNING THE REFERENCE's models/pde_loss.py SweFvLoss and models/ddim.py
PlCondEdm on the CPU.  Inputs and the reference's outputs, every file under 1 MB:

  swe_unroll.npz                 ic::<X> (3, 1, X, 2) and unroll::<system>::<X>x<n> = unroll_from_init(ic, n) for the (X, n_steps)
                                 cases of tests/_swe_unroll.py on both systems' constants, the deliberately unstable case included;
                                 loss::* = unroll_loss (flip_xy False / True, normaliser divides 0.7 / 1.3) at B 3, T 9, X 16;
                                 metric::* = print_unroll_metrics (n_samples 2, B 2, T 9, X 16, swe_per): inputs, both returned
                                 tensors and the four logged scalars
  swe_unroll_<system>_<X>x<n>.npz   unroll::<system>::<X>x<n> of the three cases whose outputs do not fit beside the others
                                 (128 x 127, 300 x 127, 4096 x 2)

Before anything is written the script asserts what the tests rely on: every case but the unstable one is finite, the unstable one
holds both NaNs and infinities on ``swe``, and a loop of oracle.pde_oracle.swe_fv_step reproduces every unrolled tensor bit for bit.

    python tools/make_golden_swe_unroll.py            # rewrites tests/golden/swe_unroll*.npz (needs the reference checkout)
    python tools/make_golden_swe_unroll.py --check    # regenerates and compares with the committed files instead
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import make_golden as mg            # noqa: E402  sets up the reference import and the Lightning stand-in

import numpy as np                  # noqa: E402
import torch                        # noqa: E402
from models.ddim import PlCondEdm   # noqa: E402  (reference)
from models.pde_loss import SweFvLoss   # noqa: E402  (reference)

from oracle import fixtures as fx   # noqa: E402
from tests import _ddpm_edm as D    # noqa: E402
from tests import _swe_unroll as U  # noqa: E402

FILES = {}


def put(fname, key, value):
    FILES.setdefault(fname, {})[key] = torch.as_tensor(value).detach().clone()


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.all((a == b) | (torch.isnan(a) & torch.isnan(b))))


def golden_unroll():
    for X in sorted({x for x, _ in U.CASES + [U.UNSTABLE]}):
        put("swe_unroll.npz", f"ic::{X}", U.initial_condition(f"ic{X}", U.B, X))
    for system, kw in U.SYSTEMS.items():
        ref = SweFvLoss(**kw)
        for X, n in U.CASES + [U.UNSTABLE]:
            ic = FILES["swe_unroll.npz"][f"ic::{X}"]
            out = ref.unroll_from_init(ic, n)
            assert tuple(out.shape) == (U.B, n + 1, X, 2) and out.dtype == torch.float32 and torch.equal(out[:, 0:1], ic)
            finite = bool(torch.isfinite(out).all())
            if (X, n) != U.UNSTABLE:
                assert finite, (system, X, n)
            elif system == "swe":               # swe_per's smaller time step survives these inputs; it is stored all the same
                assert bool(torch.isnan(out).any()) and bool(torch.isinf(out).any()), (system, X, n)
            assert same(out, U.oracle_unroll(ic, n, **kw)), (system, X, n)
            print(f"  {system:8s} X {X:5d} n_steps {n:4d}: finite {finite}, max|finite v| "
                  f"{float(out[torch.isfinite(out)].abs().max()):.4g}, NaNs {int(torch.isnan(out).sum())}")
            put(U.file_of(system, X, n), f"unroll::{system}::{X}x{n}", out)


def loss_inputs(system):
    """pred = the reference's own unroll of a smooth wave plus a perturbation (so that gt != the unroll of pred[:, 0]); gt = that
    unroll, unperturbed."""
    b, T, X = U.LOSS_SHAPE
    ref = SweFvLoss(**U.SYSTEMS[system])
    gt = ref.unroll_from_init(U.initial_condition(f"loss/{system}", b, X), T - 1)
    pred = gt + 0.02 * fx.randn(f"swe_unroll/loss/{system}/pert", b, T, X, 2)
    return pred, gt


def golden_loss():
    nh, nu = U.Norm(U.LOSS_DIVIDE[0]), U.Norm(U.LOSS_DIVIDE[1])
    for system, kw in U.SYSTEMS.items():
        pred, gt = loss_inputs(system)
        put("swe_unroll.npz", f"loss::{system}::pred", pred)
        put("swe_unroll.npz", f"loss::{system}::gt", gt)
        got = {}
        for flip in (False, True):
            ref = SweFvLoss(flip_xy=flip, **kw)
            # with flip_xy the state arrives as (u, h) and the normalisers in that order too (models/pde_loss.py:6-17, 199-209)
            p, g, a, b = (pred.flip(-1), gt.flip(-1), nu, nh) if flip else (pred, gt, nh, nu)
            loss, unrolled = ref.unroll_loss(p, g, a, b, return_unroll=True)
            assert torch.equal(loss, ref.unroll_loss(p, g, a, b)) and bool(torch.isfinite(loss).all())
            assert torch.equal(unrolled, U.oracle_unroll(pred[:, 0:1], pred.shape[1] - 1, **kw))
            put("swe_unroll.npz", f"loss::{system}::flip{int(flip)}::loss", loss)
            put("swe_unroll.npz", f"loss::{system}::flip{int(flip)}::unrolled", unrolled)
            got[flip] = loss
        # the flipped call sees the physical (h, u) state again, scaled by (divide_h, divide_u)^2 either way
        assert torch.equal(got[False], got[True])
        swapped = SweFvLoss(**kw).unroll_loss(pred, gt, nu, nh)
        assert not torch.equal(swapped, got[False])
        print(f"  unroll_loss {system}: mean {float(got[False].mean()):.4g}, max {float(got[False].max()):.4g}")


def golden_metrics():
    n, b, T, X = U.METRIC_N, U.METRIC_B, U.METRIC_T, U.METRIC_X
    st = fx.STEP_NORM_STATS
    logs = {}
    m = D.fill(PlCondEdm(mg._wrap(D.hparams_dict())), 1, st)
    m.set_pde_loss_function(U.METRIC_SYSTEM, False)
    m.log = lambda name, value, **k: logs.__setitem__(name, torch.as_tensor(value).detach().clone())
    # the truth: the solver's own run from a wave around the normaliser's mean; the recovered states: the truth plus an error
    kw = U.SYSTEMS[U.METRIC_SYSTEM]
    ic = U.initial_condition("metric", b, X)
    ic = torch.stack((st[0] + (ic[..., 0] - 1.0) * 0.5, ic[..., 1] * 0.5), dim=-1)
    truth = SweFvLoss(**kw).unroll_from_init(ic, T - 1)
    truth = truth + 0.002 * fx.randn("swe_unroll/metric/truth", b, T, X, 2)      # not the solver's own fixed point: a non-zero gt error
    h_unnorm, u_unnorm = truth[..., 0:1].contiguous(), truth[..., 1:2].contiguous()
    state_gt = m.data_transform(h_unnorm, u_unnorm)
    xs = (state_gt[..., 1:2].repeat(n, 1, 1, 1) + 0.05 * fx.randn("swe_unroll/metric/err", n * b, T, X, 1)).unsqueeze(1)
    pde_before = m.pde_loss
    with torch.no_grad():
        res, res_gt = m.print_unroll_metrics(xs, h_unnorm, u_unnorm, state_gt, n)
    assert m.pde_loss is m.pde_loss_simulator and m.pde_loss is not pde_before
    assert tuple(res.shape) == (b, 1, T, X, n, 2) and tuple(res_gt.shape) == (b, T, X, 2) and sorted(logs) == sorted(U.METRIC_LOGS)
    assert bool(torch.isfinite(res).all()) and bool(torch.isfinite(res_gt).all()) and res.dtype == torch.float32
    for k, v in (("xs", xs), ("h_unnorm", h_unnorm), ("u_unnorm", u_unnorm), ("state_gt", state_gt), ("unroll_res", res),
                 ("unroll_res_gt", res_gt)):
        put("swe_unroll.npz", f"metric::{k}", v)
    for k in U.METRIC_LOGS:
        print(f"  {k} = {float(logs[k]):.6g}")
        put("swe_unroll.npz", f"metric::log::{k}", logs[k])


if __name__ == "__main__":
    golden_unroll()
    golden_loss()
    golden_metrics()
    for fname, arrays in FILES.items():
        if "--check" in sys.argv[1:]:
            old = np.load(os.path.join(mg.OUT, fname))
            assert sorted(old.files) == sorted(arrays), fname
            for k, v in arrays.items():
                assert same(torch.from_numpy(old[k]), v), (fname, k)
            print(f"{fname}: {len(arrays)} arrays regenerate bit for bit")
        else:
            mg.save(fname, **arrays)
            assert os.path.getsize(os.path.join(mg.OUT, fname)) < 1 << 20, fname
