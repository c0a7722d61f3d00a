"""PlCondDdim (configs/model/adm_cond_h_res32.yaml: ADM U-Net ch 64, ch_mult [1, 1, 1], self_cond) at B = 32, 128 x 128 against
the EDM module of the same architecture (PlCondEdm, no self-conditioning channels), one JSON line:

  * ms per epsilon-prediction training step (training_step + backward) with the self-conditioning pre-pass forced off / on
  * ms per EDM training step of PlCondEdm
  * states/s of the 50-step VP sampler (PlCondDdim.sample_edm) and of PlCondEdm's 50-step EDM sampler (S_churn 15 both)

    python tools/cond_ddim_bench.py [steps] [B]
"""
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mcedm_amd  # noqa: E402,F401
from mcedm_amd.ddim import PlCondDdim, PlCondEdm  # noqa: E402
from oracle import mcedm_oracle as orc  # noqa: E402
from tests.test_cond_ddim_cpu import ddim_hparams  # noqa: E402

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
B = int(sys.argv[2]) if len(sys.argv) > 2 else 32
S = 128
dev = torch.device("cuda", 0)
gen = torch.Generator().manual_seed(3)


def filled(m, cfg):
    P = orc.make_params(cfg, 5)
    with torch.no_grad():
        for net in (m.model, m.ema_model.ma_model):
            for n, p in net.named_parameters():
                p.copy_(P[n])
    return m.to(dev)


def timed(fn, n):
    fn()
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


h = (torch.randn(B, S, S, 1, generator=gen) * 0.2 + 1.4).to(dev)
u = (torch.randn(B, S, S, 1, generator=gen) * 0.5).to(dev)
un = torch.randn(B, S, S, 1, generator=gen).to(dev)
batch = (h, None, None, u)
ddim = filled(PlCondDdim(ddim_hparams(timesteps=50)), orc.UNetConfig(in_channels=1, cond_channels=2, out_ch=1))
hp = ddim_hparams(name="adm_edm_cond_h", self_cond=False)
edm = filled(PlCondEdm(hp), orc.UNetConfig(in_channels=1, cond_channels=1, out_ch=1))
real_rand = torch.rand


def eps_step(sc):
    draws = [torch.tensor([0.5]), torch.tensor([0.2 if sc else 0.7])]      # cond_p 1: conditioning on; then the pre-pass draw
    torch.rand = lambda *a, **k: draws.pop(0)
    try:
        loss = ddim.training_step(batch, 0)
    finally:
        torch.rand = real_rand
    loss.backward()


def edm_step():
    edm.training_step(batch, 0).backward()


out = {"B": B, "H": S, "W": S,
       "eps_step_ms_no_selfcond": timed(lambda: eps_step(False), steps),
       "eps_step_ms_selfcond": timed(lambda: eps_step(True), steps),
       "edm_step_ms": timed(edm_step, steps)}
with torch.no_grad():
    fwd = lambda: ddim.model(u.permute(0, 3, 1, 2).contiguous(), torch.full((B,), 500.0, device=dev))   # noqa: E731
    out["forward_ms"] = timed(fwd, steps)
sp = ddim.sparams
ddim.set_test_sampler_params(sp)
n_s = max(1, steps // 5)
out["vp_sampler_states_per_s"] = B / (timed(lambda: ddim.sample_edm(h, un, sp), n_s) / 1e3)
out["edm_sampler_states_per_s"] = B / (timed(lambda: edm.sample_edm(h, un, sp), n_s) / 1e3)
print(json.dumps(out))
