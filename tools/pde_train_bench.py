"""The PDE term of training (mcedm_pde_train_loss) at B = 32, 128 x 128, one JSON line:

  * us per launch of its kernels for both systems, value + gradient and value alone (mcedm_prof_enable / _report: HIP events
    around each launch), with the algorithmic bytes over that time
  * ms per PlCondEdm training step (training_step + backward, ADM U-Net ch 64) with pde_loss_lambda > 0 next to lambda = 0 on the
    same build, the two alternating, and the kernel list of one lambda = 0 step (names and launch counts)

    python tools/pde_train_bench.py [steps] [B]
"""
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mcedm_amd  # noqa: E402,F401
from mcedm_amd import lib as L  # noqa: E402
from mcedm_amd.ddim import PlCondEdm  # noqa: E402
from mcedm_amd.pde_loss import get_pde_loss_function  # noqa: E402
from mcedm_amd.pl_base import Normalizer  # noqa: E402
from oracle import mcedm_oracle as orc  # noqa: E402
from tests.test_cond_ddim_cpu import ddim_hparams  # noqa: E402

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
B = int(sys.argv[2]) if len(sys.argv) > 2 else 32
S = 128
STATS = (1.4, 0.2, 0.0, 0.5)
dev = torch.device("cuda", 0)
gen = torch.Generator().manual_seed(3)
h = (torch.randn(B, S, S, 1, generator=gen) * 0.2 + 1.4).to(dev)
u = (torch.randn(B, S, S, 1, generator=gen) * 0.5).to(dev)
out = {"B": B, "H": S, "W": S, "kernels_us": {}}

# ---- the entry alone
nh, nu = Normalizer(()), Normalizer(())
nh.set_stats(torch.tensor(STATS[0]), torch.tensor(STATS[1]))
nu.set_stats(torch.tensor(STATS[2]), torch.tensor(STATS[3]))
hn, D = ((h - STATS[0]) / STATS[1]).contiguous(), ((u - STATS[2]) / STATS[3]).permute(0, 3, 1, 2).contiguous()
for system in ("swe_per", "darcy"):
    gd = get_pde_loss_function(system, False)[0].guidance_desc(nh, nu, S, S, weight=0.1)
    for tag, dD in (("value_and_grad", torch.zeros_like(D)), ("value", None)):
        for _ in range(3):
            L.pde_train_loss(gd, D, hn, dD=dD)
        torch.cuda.synchronize()
        L.prof_enable(True)
        for _ in range(steps):
            L.pde_train_loss(gd, D, hn, dD=dD)
        rows = L.prof_report()
        L.prof_enable(False)
        out["kernels_us"][f"{system}/{tag}"] = {r["name"]: {"us_per_launch": r["total_ms"] / r["launches"] * 1e3,
                                                             "GB_per_s": r["bytes"] / r["launches"] / (r["total_ms"] / r["launches"] * 1e-3) / 1e9}
                                                for r in rows}


# ---- the training step with and without the term
def module(lam):
    hp = ddim_hparams(name="adm_edm_cond_h", self_cond=False)
    hp.optimization.pde_loss_lambda = lam
    m = PlCondEdm(hp)
    P = orc.make_params(orc.UNetConfig(in_channels=1, cond_channels=1, out_ch=1), 5)
    with torch.no_grad():
        for net in (m.model, m.ema_model.ma_model):
            for n, p in net.named_parameters():
                p.copy_(P[n])
    m = m.to(dev)
    m.normalizer_input.set_stats(torch.tensor(STATS[0]), torch.tensor(STATS[1]))
    m.normalizer_target.set_stats(torch.tensor(STATS[2]), torch.tensor(STATS[3]))
    m.set_pde_loss_function("swe_per", False)
    return m


mods = {"lambda0": module(0.0), "lambda0.1": module(0.1)}
batch = (h, None, None, u)


def step(m):
    m.training_step(batch, 0).backward()


for m in mods.values():
    for _ in range(3):
        step(m)
torch.cuda.synchronize()
times = {k: [] for k in mods}
for _ in range(5):                                     # alternate the two: other work shares the host
    for k, m in mods.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            step(m)
        torch.cuda.synchronize()
        times[k].append((time.perf_counter() - t0) / steps * 1e3)
out["train_step_ms"] = {k: {"median": sorted(v)[len(v) // 2], "min": min(v), "max": max(v)} for k, v in times.items()}
L.prof_enable(True)
step(mods["lambda0"])
out["lambda0_step_kernels"] = {r["name"]: r["launches"] for r in L.prof_report()}
L.prof_enable(False)
print(json.dumps(out))
