"""The DDIM sampler of PlCondDdim (configs/model/adm_cond_h_res32.yaml: ADM U-Net ch 64, ch_mult [1, 1, 1], self_cond) at B = 32,
128 x 128 on one MI355X, one JSON line:

  * the 50-step configs/diff_sampler/default.yaml call (type ddim, uniform, eta 0, w 0) next to the 50-step sample_edm of
    the same module, ms per call (host clock around calls that end in a device synchronise, warmed up);
  * the fused step kernel on its own (guided, stochastic, both trajectory slots: 36 bytes per element), device events around
    a replayed HIP graph of 100 back-to-back launches (kernel boundaries included): us per launch, GB/s and the share of the 8 TB/s HBM peak.  Its 19 MB working set
    stays in the 256 MiB Infinity Cache between launches, so the figure is a rate of the kernel, not of HBM.

    python tools/cond_ddim_sample_bench.py [calls] [B] [out.json]
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
from mcedm_amd.ddim import PlCondDdim  # noqa: E402
from mcedm_amd.pl_base import DotDict  # noqa: E402
from oracle import mcedm_oracle as orc  # noqa: E402
from tests.test_cond_ddim_cpu import ddim_hparams  # noqa: E402

calls = int(sys.argv[1]) if len(sys.argv) > 1 else 3
B = int(sys.argv[2]) if len(sys.argv) > 2 else 32
S = 128
dev = torch.device("cuda", 0)
gen = torch.Generator().manual_seed(3)


def timed(fn, n):
    fn()
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


m = PlCondDdim(ddim_hparams(timesteps=50))
P = orc.make_params(orc.UNetConfig(in_channels=1, cond_channels=2, out_ch=1), 5)
with torch.no_grad():
    for net in (m.model, m.ema_model.ma_model):
        for n, p in net.named_parameters():
            p.copy_(P[n])
m = m.to(dev)
h = (torch.randn(B, S, S, 1, generator=gen) * 0.2 + 1.4).to(dev)
un = torch.randn(B, S, S, 1, generator=gen).to(dev)
ddim_sp = DotDict(name="ddim_1_sample", type="ddim", timesteps=50, skip_type="uniform", eta=0.0, n_samples=1, n_repeat=5,
                  n_time_h=128, n_time_u=0, return_last=True, select_by_pde=False, use_gt_pde_select=True, guide_dx=False, w=0.0,
                  plot_scaled=False)
edm_sp = m.sparams
m.set_test_sampler_params(edm_sp)
out = {"B": B, "H": S, "W": S, "steps": 50}
out["ddim_sample_ms"] = timed(lambda: m.sample(h, un, ddim_sp), calls)
out["sample_edm_ms"] = timed(lambda: m.sample_edm(h, un, edm_sp), calls)

# the step kernel alone
shape = (B, 1, S, S)
xt, F, Fu = (torch.randn(shape, generator=gen).to(dev) for _ in range(3))
nz = torch.rand(shape, generator=gen).to(dev)
condp, condu = torch.zeros(B, 2, S, S, device=dev), torch.zeros(B, 2, S, S, device=dev)
xs, x0s = torch.empty(B, 51, S, S, 1, device=dev), torch.empty(B, 50, S, S, 1, device=dev)
step = lambda k: L.op_ddim_cond_step(xt, F, 0.6, 0.8, 0.7, 0.5, Fu=Fu, w=0.5, noise=nz, c1=0.3, condp=condp, condp_u=condu,  # noqa: E731
                                     cond_channels=1, xs=xs, t_xs=k % 50 + 1, x0s=x0s, t_x0=k % 50)
n_launch, reps = 100, 10
graph = L._capture(lambda: [step(k) for k in range(n_launch)], dev)      # a replayed train: no host time between the launches
graph.replay()
torch.cuda.synchronize()
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
e0.record()
for _ in range(reps):
    graph.replay()
e1.record()
torch.cuda.synchronize()
us = e0.elapsed_time(e1) * 1e3 / (n_launch * reps)
n_el = B * S * S
out["step_kernel"] = {"bytes_per_element": 36, "elements": n_el, "us_per_launch_back_to_back": us,
                      "GBps": 36 * n_el / us * 1e-3, "share_of_8TBps_hbm_peak": 36 * n_el / (us * 1e-6) / 8e12}
line = json.dumps(out)
print(line)
if len(sys.argv) > 3:
    with open(sys.argv[3], "w") as f:
        f.write(line + "\n")
