"""What tools/make_golden_swe_unroll.py (the reference's runs, CPU) and the tests of the device-side SWE unroll share: the two
systems' constants, the (X, n_steps) cases, the form of the inputs and the names of the fixture's entries.  The inputs themselves
and the reference's outputs live in tests/golden/swe_unroll*.npz.

The FORCE scheme is only conditionally stable: with h = 1 + 0.3 sin(2 pi (x + phi)) + 0.01 randn, u = 0.2 cos(2 pi (x + phi)) +
0.01 randn the reference's unroll stays finite for n_steps >= X / 3 on ``swe`` and n_steps >= X / 6 on ``swe_per``, and for
n_steps <= 2 at any X; every bit-equality case lies inside those bounds, and UNSTABLE is the one case that deliberately does not."""
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import fixtures as fx  # noqa: E402

# get_pde_loss_function (models/loss_helper.py:14-38): constructor arguments of SweFvLoss per system
SYSTEMS = {"swe": dict(Tn=1.28, x_min=-2.5, x_max=2.5), "swe_per": dict(Tn=0.128, x_min=-0.5, x_max=0.5)}
B = 3
# (X, n_steps): one cell / narrower than the stencil / as wide as it, odd steps / odd X / one wave / one cell past a wave / the
# reference's own shape / more cells than a small workgroup / the LDS limit (the cell loop)
CASES = [(1, 1), (2, 2), (3, 7), (5, 16), (64, 32), (65, 33), (128, 127), (300, 127), (4096, 2)]
UNSTABLE = (128, 16)
# the cases whose outputs are too large to share one file under the repository's size limit get a file of their own
BIG = {(128, 127), (300, 127), (4096, 2)}
LOSS_SHAPE = (3, 9, 16)                 # B, T, X of the unroll_loss cases
LOSS_DIVIDE = (0.7, 1.3)                # normalizer_h.divide, normalizer_u.divide: different, so a swapped scale shows
METRIC_N, METRIC_B, METRIC_T, METRIC_X = 2, 2, 9, 16
METRIC_SYSTEM = "swe_per"
METRIC_LOGS = ("test_pde_unroll_error", "test_pde_unroll_error_gt", "test_pde_unrolled_mae_h", "test_pde_unrolled_mae_u")


def file_of(system, X, n_steps):
    return f"swe_unroll_{system}_{X}x{n_steps}.npz" if (X, n_steps) in BIG else "swe_unroll.npz"


def initial_condition(tag, b, X):
    """(b, 1, X, 2) = (h, u): a smooth wave of random phase plus a little noise."""
    x = torch.linspace(0, 1, X).view(1, 1, X)
    ph = torch.from_numpy(fx.uniform(f"swe_unroll/{tag}/phase", b, 1, 1)).to(torch.float32)
    h = 1.0 + 0.3 * torch.sin(2 * math.pi * (x + ph)) + 0.01 * fx.randn(f"swe_unroll/{tag}/h", b, 1, X)
    u = 0.2 * torch.cos(2 * math.pi * (x + ph)) + 0.01 * fx.randn(f"swe_unroll/{tag}/u", b, 1, X)
    return torch.stack((h, u), dim=-1)


class Norm:
    """The two attributes of models/normalizer.py:Normalizer that the losses read."""

    def __init__(self, divide, device="cpu"):
        self.subtract = torch.tensor(0.0, device=device)
        self.divide = torch.tensor(divide, device=device)


def oracle_unroll(ic, n_steps, Tn, x_min, x_max):
    """unroll_from_init as a loop of the oracle's step."""
    from oracle import pde_oracle as po
    rows, cur = [ic], ic
    for _ in range(n_steps):
        cur = po.swe_fv_step(cur, Tn / n_steps, x_min, x_max)
        rows.append(cur)
    return torch.cat(rows, dim=1)
