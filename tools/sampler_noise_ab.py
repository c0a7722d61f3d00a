"""Where the samplers' per-step noise comes from, measured: `PlCondDdim.sample_edm` and `PlCondEdm.sample_edm` on the shipped
network (ADM U-Net ch 64, ch_mult [1, 1, 1], attention at 32, 128 x 128, B = 32) with the shipped sampler (50 steps, S_churn 15),
ms per call and peak allocation for `noise_source` "torch" and "device", on one MI355X.

    python tools/sampler_noise_ab.py ab OUT.json [--trees NAME=DIR ...] [--rounds R] [--reps N]
        Every (tree, module, noise source) runs in a child process of its own (the peak allocation of one configuration must not
        hold another's buffers), the trees alternating within each round, so that two checkouts built side by side -- this one
        and its parent commit -- are compared on the same card in the same call.  Default: this tree alone.  Per configuration:
        median, min and max over all timed calls of all rounds, the rounds' medians (run-to-run spread), peak bytes.
    python tools/sampler_noise_ab.py one MODULE SOURCE [--reps N]           (what a child runs; one JSON line)
    python tools/sampler_noise_ab.py kernels cond_noise | cond_rng | next    (under `rocprofv3 --kernel-trace --stats -- python ...`)
        The two DDIM step kernels with their uniform draws read from a tensor and generated in the kernel, 20 launches each
        at B = 32, 128 x 128: ddim_cond_step_kernel through its op entry (one kernel name for both forms, hence one rocprofv3
        command per form), ddim_next_kernel and ddim_next_rng_kernel through a 20-step mcedm_ddim_repaint_sample and
        mcedm_ddim_repaint_sample_rng on the res-128 DDPM U-Net (`next`: both names in one trace).
"""
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROOT = os.path.abspath(os.environ.get("MCEDM_AB_TREE", HERE))           # the checkout whose package is measured
B, S, STEPS, CHURN = 32, 128, 50, 15.0


def hparams(DotDict, name, self_cond):
    wrap = lambda d: DotDict({k: wrap(v) for k, v in d.items()}) if isinstance(d, dict) else d      # noqa: E731
    return wrap(dict(
        name=name,
        model=dict(type="simple", in_channels=1, cond_channels=1, cat_cond=True, out_ch=1, ch=64, ch_mult=[1, 1, 1], num_res_blocks=1,
                   attn_resolutions=[32], dropout=0.0, label_dim=0, augment_dim=0, label_dropout=0, ema_rate=0.999, ema=True,
                   resamp_with_conv=True, resolution=128, self_cond=self_cond, cond_p=1.0, dx_cond=False, cat_dx=False, dx_norm="l2",
                   dx_detach=False, add_cond_mask=False, add_xt=False, var_type="fixedsmall", node_type=False),
        data=dict(normalization="gauss", uniform_dequantization=False, gaussian_dequantization=False, rescaled=False),
        diffusion=dict(beta_schedule="linear", beta_start=0.0001, beta_end=0.02, num_diffusion_timesteps=1000),
        optimization=dict(optimizer="Adam", lr=0.0002, weight_decay=0.0, beta1=0.9, amsgrad=False, eps=1e-8, grad_clip=1.0, loss="l2",
                          pde_loss_lambda=0.0, pde_loss_prop_t=False, use_gt_pde=False, factor=0.3, step_size=50),
        sampler=dict(name="edm", type="edm", timesteps=STEPS, sigma_min=0.002, sigma_max=80, rho=7, S_churn=CHURN, S_min=0,
                     S_max="inf", S_noise=1, n_samples=1, n_repeat=2, n_time_h=128, n_time_u=0, return_last=True, select_by_pde=False,
                     use_gt_pde_select=True, guide_dx=False, w=0.0, plot_scaled=False)))


def one(module, source, reps):
    sys.path.insert(0, ROOT)
    import torch
    import mcedm_amd  # noqa: F401
    from mcedm_amd import ddim
    from mcedm_amd.pl_base import DotDict
    from oracle import mcedm_oracle as orc
    assert torch.cuda.is_available(), "this measurement needs the MI355X"
    dev = torch.device("cuda", 0)
    cls, self_cond = {"PlCondDdim": (ddim.PlCondDdim, True), "PlCondEdm": (ddim.PlCondEdm, False)}[module]
    m = cls(hparams(DotDict, "adm_cond_h" if self_cond else "adm_edm_cond_h", self_cond))
    P = orc.make_params(orc.UNetConfig(in_channels=1, cond_channels=2 if self_cond else 1, out_ch=1), 5)
    with torch.no_grad():
        for net in (m.model, m.ema_model.ma_model):
            for n, p in net.named_parameters():
                p.copy_(P[n])
    m = m.to(dev)
    m.noise_source = source                      # (a checkout from before the attribute existed ignores it)
    gen = torch.Generator().manual_seed(3)
    h = (torch.randn(B, S, S, 1, generator=gen) * 0.2 + 1.4).to(dev)
    un = torch.randn(B, S, S, 1, generator=gen).to(dev)
    sp = m.sparams
    m.set_test_sampler_params(sp)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    torch.manual_seed(0)
    for _ in range(2):                           # the first call captures the graph where the checkout replays one
        out = m.sample_edm(h, un, sp, return_last=True)
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = m.sample_edm(h, un, sp, return_last=True)
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    assert bool(torch.isfinite(out).all())
    print(json.dumps({"module": module, "noise_source": source, "ms": times, "peak_bytes": torch.cuda.max_memory_allocated(),
                      "allocated_before_bytes": base, "graphs": len(getattr(m, "_graphs", {}))}))


def ab(out_path, trees, rounds, reps):
    # a checkout from before the single-task modules had the switch draws with torch whatever the attribute says: one row for it
    has_switch = {t: "MCEDM_NOISE_SOURCE" in open(os.path.join(d, "m-cedm_amd", "ddim.py")).read() for t, d in trees.items()}
    configs = [(t, mod, src) for mod in ("PlCondDdim", "PlCondEdm") for src in ("torch", "device") for t in trees
               if has_switch[t] or src == "torch"]
    runs = {c: [] for c in configs}
    for r in range(rounds):
        for c in configs:
            env = dict(os.environ, MCEDM_AB_TREE=trees[c[0]])
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "one", c[1], c[2], "--reps", str(reps)], env=env,
                               capture_output=True, text=True, timeout=400)
            if p.returncode != 0:                # nothing more is started on the card after a failed child
                sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                raise SystemExit(f"{c}: child exited with {p.returncode}")
            runs[c].append(json.loads(p.stdout.strip().splitlines()[-1]))
            print(c, f"round {r}: median {statistics.median(runs[c][-1]['ms']):.1f} ms", flush=True)
    rows = []
    for c, rs in runs.items():
        ms = [v for r in rs for v in r["ms"]]
        rows.append({"tree": c[0], "module": c[1], "noise_source": c[2], "calls": len(ms), "median_ms": statistics.median(ms),
                     "min_ms": min(ms), "max_ms": max(ms), "round_medians_ms": [statistics.median(r["ms"]) for r in rs],
                     "peak_bytes": max(r["peak_bytes"] for r in rs), "allocated_before_bytes": rs[0]["allocated_before_bytes"],
                     "graphs": rs[0]["graphs"]})
    res = {"B": B, "H": S, "W": S, "timesteps": STEPS, "S_churn": CHURN, "noise_tensor_bytes": STEPS * B * S * S * 8, "rows": rows}
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


def kernels(which):
    sys.path.insert(0, ROOT)
    import torch
    import mcedm_amd  # noqa: F401
    from mcedm_amd import lib as L
    dev = torch.device("cuda", 0)
    gen = torch.Generator().manual_seed(3)
    seed = torch.tensor([5], dtype=torch.int64, device=dev)
    if which in ("cond_noise", "cond_rng"):
        shape = (B, 1, S, S)
        xt, F, Fu = (torch.randn(shape, generator=gen).to(dev) for _ in range(3))
        nz = torch.rand(shape, generator=gen).to(dev)
        condp, condu = torch.zeros(B, 2, S, S, device=dev), torch.zeros(B, 2, S, S, device=dev)
        xs, x0s = torch.empty(B, 21, S, S, 1, device=dev), torch.empty(B, 20, S, S, 1, device=dev)
        kw = dict(noise=nz) if which == "cond_noise" else dict(rng_seed=seed)
        for k in range(20):
            L.op_ddim_cond_step(xt, F, 0.6, 0.8, 0.7, 0.5, Fu=Fu, w=0.5, c1=0.3, condp=condp, condp_u=condu, cond_channels=1, xs=xs,
                                t_xs=k + 1, x0s=x0s, t_x0=k, **(dict(kw, draw=k) if which == "cond_rng" else kw))
    else:
        from oracle import ddpm_oracle as dorc
        cfg = dorc.DdpmConfig()
        plan = L.DdpmPlan(cfg.in_channels, cfg.out_ch, cfg.ch, cfg.ch_mult, cfg.num_res_blocks, cfg.attn_resolutions, cfg.resolution)
        packed = plan.pack({k: v.to(dev) for k, v in dorc.make_params(cfg, 21).items()}, dorc.timestep_freqs(cfg.ch).to(dev))
        sp = dorc.DdimParams(timesteps=20, skip_type="uniform", eta=0.01, n_repeat=1, n_time_h=0, n_time_u=64)
        dd, keep = L.ddim_desc(sp, dorc.alphas_ext_of(dorc.betas_of(cfg)), 1, 1, True)
        hu = torch.randn(B, 2, S, S, generator=gen).to(dev)
        init = torch.randn(B, 2, S, S, generator=gen).to(dev)
        eta = torch.rand(20, B, 2, S, S, generator=gen).to(dev)
        plan.ddim_repaint_sample(packed, dd, hu, init, eta)                      # ddim_next_kernel
        plan.ddim_repaint_sample(packed, dd, hu, init, rng_seed=seed)            # ddim_next_rng_kernel
    torch.cuda.synchronize()


if __name__ == "__main__":
    a = sys.argv[1:]
    opt = lambda k, d: a[a.index(k) + 1] if k in a else d      # noqa: E731
    if a and a[0] == "one":
        one(a[1], a[2], int(opt("--reps", 5)))
    elif a and a[0] == "ab":
        trees = {"this": HERE}
        if "--trees" in a:
            trees = dict(t.split("=", 1) for t in a[a.index("--trees") + 1:] if "=" in t)
        ab(a[1], {k: os.path.abspath(v) for k, v in trees.items()}, int(opt("--rounds", 2)), int(opt("--reps", 5)))
    elif a and a[0] == "kernels":
        kernels(a[1])
    else:
        raise SystemExit(__doc__)
