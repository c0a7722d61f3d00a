"""PlCondDdim on the DDPM U-Net with the cond_enc head (configs/model/ddim_cond_h_res32.yaml: ch 64, ch_mult [1, 1, 1], self_cond) at
B = 32, 128 x 128 on one MI355X, one JSON line:

  * ms per network evaluation of the conditioned plan (folded conv_in + the map as its residual) next to the same architecture's
    plan WITHOUT the head (mcedm_ddpm_forward_sc: the launches a network evaluation had before the head existed), alternated in
    one process, `rounds` rounds of `evals` evaluations each, device events around each train; the ratio per round and its spread;
  * ms of the map kernel (device events around a train of launches);
  * states/s of the shipped 50-step sample_edm (S_churn 15, w 0; host clock around calls that end in a device synchronise).

    python tools/ddpm_cond_bench.py [rounds] [B] [out.json]
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

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
B = int(sys.argv[2]) if len(sys.argv) > 2 else 32
S, evals = 128, 20
dev = torch.device("cuda", 0)
torch.manual_seed(3)


def wrap(d):
    return DotDict({k: wrap(v) for k, v in d.items()}) if isinstance(d, dict) else d


sampler = dict(name="edm", type="edm", timesteps=50, sigma_min=0.002, sigma_max=80, rho=7, S_churn=15.0, S_min=0, S_max="inf", S_noise=1,
               n_samples=1, n_repeat=2, n_time_h=128, n_time_u=0, return_last=True, select_by_pde=False, use_gt_pde_select=True,
               guide_dx=False, w=0.0, plot_scaled=False)
hp = wrap(dict(
    name="ddim_cond_h",
    model=dict(type="simple", in_channels=1, cond_channels=1, cat_cond=False, out_ch=1, ch=64, ch_mult=[1, 1, 1], num_res_blocks=1,
               attn_resolutions=[32], dropout=0.0, var_type="fixedsmall", ema_rate=0.999, ema=True, resamp_with_conv=True, resolution=S,
               self_cond=True, cond_p=1.0, dx_cond=False, cat_dx=False, dx_norm="l2", dx_detach=False, node_type=False),
    data=dict(normalization="gauss", uniform_dequantization=False, gaussian_dequantization=False, rescaled=False),
    diffusion=dict(beta_schedule="linear", beta_start=0.0001, beta_end=0.02, num_diffusion_timesteps=1000),
    optimization=dict(optimizer="Adam", lr=0.0002, weight_decay=0.0, beta1=0.9, amsgrad=False, eps=1e-8, grad_clip=1.0, loss="l2",
                      pde_loss_lambda=0.0, pde_loss_prop_t=False, use_gt_pde=False, factor=0.3, step_size=50),
    sampler=sampler))
m = PlCondDdim(hp).to(dev)
net = m.ema_model.ma_model
plain = L.DdpmPlan(1, 1, 64, (1, 1, 1), 1, (32,), S, self_cond=True)
x, xsc, cond = (torch.randn(B, 1, S, S, device=dev) for _ in range(3))


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
    params = {k: v for k, v in net.named_parameters() if not k.startswith(("cond_enc", "combine_enc"))}
    pk_plain = plain.pack(params, net.timestep_freqs(dev))
    ws_c, ws_p = L.Workspace(), L.Workspace()
    cmap = net.plan.cond_map(pk, cond)
    f_cond = lambda: net.plan.forward_cond(pk, x, 500.0, cond_map=cmap, x_self_cond=xsc, ws=ws_c)      # noqa: E731
    f_none = lambda: net.plan.forward_cond(pk, x, 500.0, x_self_cond=xsc, ws=ws_c)                     # noqa: E731
    f_plain = lambda: plain.forward(pk_plain, x, 500.0, ws=ws_p, x_self_cond=xsc)                      # noqa: E731
    f_map = lambda: net.plan.cond_map(pk, cond, out=cmap)                                              # noqa: E731
    for f in (f_cond, f_none, f_plain, f_map):
        train_ms(f, 3)                                                                                 # warm-up
    rows = []
    for _ in range(rounds):                                                                            # alternated, same process
        rows.append({"plain_ms": train_ms(f_plain, evals), "cond_ms": train_ms(f_cond, evals), "cond_none_ms": train_ms(f_none, evals),
                     "map_ms": train_ms(f_map, evals)})
    out = {"B": B, "H": S, "W": S, "evals_per_round": evals, "rounds": rows}
    for k in ("plain_ms", "cond_ms", "cond_none_ms", "map_ms"):
        v = sorted(r[k] for r in rows)
        out[k] = {"median": v[len(v) // 2], "min": v[0], "max": v[-1]}
    ratios = sorted(r["cond_ms"] / r["plain_ms"] for r in rows)
    out["cond_over_plain"] = {"median": ratios[len(ratios) // 2], "min": ratios[0], "max": ratios[-1]}
    out["predicted_cond_over_plain"] = 1.0 + 4.2 / 230.0

    m.set_test_sampler_params(m.sparams)
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
if len(sys.argv) > 3:
    with open(sys.argv[3], "w") as f:
        f.write(line + "\n")
