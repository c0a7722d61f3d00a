"""PlCondEdm on the DDPM U-Net with the conditioning concatenated to its input (configs/model/edm_cond_h_res32.yaml: ch 64,
ch_mult [1, 1, 1], cat_cond, no self-conditioning) at B = 32, 128 x 128 on one MI355X, one JSON line:

  * ms per conditioned denoiser call (mcedm_ddpm_edm_denoise, w 0: conv_in reads two planes) next to mcedm_ddpm_denoise on the same
    architecture's plan WITHOUT cond (conv_in reads one plane), alternated in one process, `rounds` rounds of `evals` calls each,
    device events around each train; the ratio per round and its spread;
  * states/s of the shipped 50-step sample_edm (S_churn 15, w 0; host clock around calls that end in a device synchronise).

    python tools/ddpm_edm_bench.py [rounds] [B] [out.json]      # out.json defaults to profiles/ddpm_edm_bench.json
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
from mcedm_amd.pl_base import DotDict  # noqa: E402

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
B = int(sys.argv[2]) if len(sys.argv) > 2 else 32
dest = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "ddpm_edm_bench.json")
S, evals = 128, 20
dev = torch.device("cuda", 0)
torch.manual_seed(3)


def wrap(d):
    return DotDict({k: wrap(v) for k, v in d.items()}) if isinstance(d, dict) else d


sampler = dict(name="edm", type="edm", timesteps=50, sigma_min=0.002, sigma_max=80, rho=7, S_churn=15.0, S_min=0, S_max="inf", S_noise=1,
               n_samples=1, n_repeat=2, n_time_h=128, n_time_u=0, return_last=True, select_by_pde=False, use_gt_pde_select=True,
               guide_dx=False, w=0.0, plot_scaled=False)
hp = wrap(dict(
    name="edm_cond_h",
    model=dict(type="simple", in_channels=1, cond_channels=1, cat_cond=True, out_ch=1, ch=64, ch_mult=[1, 1, 1], num_res_blocks=1,
               attn_resolutions=[32], dropout=0.0, var_type="fixedsmall", ema_rate=0.999, ema=True, resamp_with_conv=True, resolution=S,
               self_cond=False, cond_p=1.0, dx_cond=False, cat_dx=False, dx_norm="l2", dx_detach=False, node_type=False),
    data=dict(normalization="gauss", uniform_dequantization=False, gaussian_dequantization=False, rescaled=False),
    diffusion=dict(beta_schedule="linear", beta_start=0.0001, beta_end=0.02, num_diffusion_timesteps=1000),
    optimization=dict(optimizer="Adam", lr=0.0002, weight_decay=0.0, beta1=0.9, amsgrad=False, eps=1e-8, grad_clip=1.0, loss="l2",
                      pde_loss_lambda=0.0, pde_loss_prop_t=False, use_gt_pde=False, factor=0.3, step_size=50),
    sampler=sampler))
m = PlCondEdm(hp).to(dev)
net = m.ema_model.ma_model
plain = L.DdpmPlan(1, 1, 64, (1, 1, 1), 1, (32,), S, self_cond=False)
x, cond = (torch.randn(B, 1, S, S, device=dev) for _ in range(2))


def train_ms(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


with torch.no_grad():
    pk = net.packed_weights()
    params = {k: v.detach() for k, v in net.named_parameters()}
    params["conv_in.weight"] = params["conv_in.weight"][:, 1:].contiguous()
    pk_plain = plain.pack(params, net.timestep_freqs(dev))
    ws_c, ws_p = L.Workspace(), L.Workspace()
    sigma, c_noise = 1.3, float(torch.tensor(1.3).log() / 4)
    f_edm = lambda: net.plan.edm_denoise(pk, x, sigma, c_noise, cond=cond, ws=ws_c)      # noqa: E731
    f_plain = lambda: plain.denoise(pk_plain, x, sigma, c_noise, ws=ws_p)                # noqa: E731
    for f in (f_edm, f_plain):
        train_ms(f, 3)                                                                   # warm-up
    rows = []
    for _ in range(rounds):                                                              # alternated, same process
        rows.append({"plain_ms": train_ms(f_plain, evals), "edm_cond_ms": train_ms(f_edm, evals)})
    out = {"B": B, "H": S, "W": S, "evals_per_round": evals, "rounds": rows}
    for k in ("plain_ms", "edm_cond_ms"):
        v = sorted(r[k] for r in rows)
        out[k] = {"median": v[len(v) // 2], "min": v[0], "max": v[-1]}
    ratios = sorted(r["edm_cond_ms"] / r["plain_ms"] for r in rows)
    out["edm_cond_over_plain"] = {"median": ratios[len(ratios) // 2], "min": ratios[0], "max": ratios[-1]}

    h, un = torch.randn(B, S, S, 1, device=dev), torch.randn(B, S, S, 1, device=dev)
    call = lambda: m.sample_edm(h, un, m.sparams)      # noqa: E731
    call()
    call()
    torch.cuda.synchronize()
    t = []
    for _ in range(3):
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        t.append(time.perf_counter() - t0)
    out["sample_edm_50_steps"] = {"seconds": sorted(t), "states_per_s": B / sorted(t)[1], "noise_source": m.noise_source}
line = json.dumps(out)
print(line)
os.makedirs(os.path.dirname(os.path.abspath(dest)), exist_ok=True)
with open(dest, "w") as f:
    f.write(line + "\n")
