#!/usr/bin/env python
"""One timestep per sample on the DDPM U-Net against one for the batch, at the shipped shape (configs/model/ddim_res32.yaml: ch 64,
ch_mult (1, 1, 1), attention at 32 x 32, 128 x 128, self-conditioning; B = 32): mcedm_ddpm_forward_sc and mcedm_ddpm_forward_t
with 32 distinct timesteps, ALTERNATED inside one process, each call timed with device events after a warm-up; then the
timestep kernels' own time from the library's profiler rows.

What it answers: is the difference between the two entries accounted for by the batched timestep kernel, within the spread of
the scalar forward against itself?  Writes one JSON file (default profiles/ddpm_pert_bench.json).

    python tools/ddpm_pert_bench.py [--rounds 20] [--warmup 3] [--batch 32] [--out profiles/ddpm_pert_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import mcedm_amd  # noqa: E402,F401
from mcedm_amd import lib as L  # noqa: E402
from oracle import ddpm_oracle as ddo  # noqa: E402


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def stats(v):
    return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "stdev_ms": statistics.pstdev(v), "n": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ddpm_pert_bench.json"))
    args = ap.parse_args()
    cfg = ddo.DdpmConfig()
    B, R = args.batch, cfg.resolution
    plan = L.DdpmPlan(cfg.in_channels, cfg.out_ch, cfg.ch, cfg.ch_mult, cfg.num_res_blocks, cfg.attn_resolutions, R, self_cond=True)
    P = ddo.make_params(cfg, 5)
    packed = plan.pack({k: v.cuda() for k, v in P.items()}, ddo.timestep_freqs(cfg.ch).cuda())
    g = torch.Generator().manual_seed(11)
    x = torch.randn(B, cfg.in_channels, R, R, generator=g).cuda()
    xsc = torch.randn(B, cfg.in_channels, R, R, generator=g).cuda()
    t = torch.linspace(0, 999, B).round().cuda()
    ws = L.Workspace()
    ws.get(plan.workspace_bytes_t(B), x.device)
    scalar = lambda: plan.forward(packed, x, 500.0, ws=ws, x_self_cond=xsc)
    batched = lambda: plan.forward_t(packed, x, t, x_self_cond=xsc, ws=ws)
    for _ in range(args.warmup):
        scalar(), batched()
    torch.cuda.synchronize()
    a, b, c = [], [], []
    for _ in range(args.rounds):              # scalar, per-sample, scalar again: the second scalar series is the yardstick's own spread
        a.append(timed(scalar))
        b.append(timed(batched))
        c.append(timed(scalar))
    rows = {}
    for name, fn in (("scalar", scalar), ("per_sample", batched)):
        L.prof_enable(True)
        try:
            for _ in range(5):
                fn()
            torch.cuda.synchronize()
            rep = L.prof_report()
        finally:
            L.prof_enable(False)
        rows[name] = {r["name"]: r["total_ms"] / r["launches"] for r in rep}
    temb_ms = rows["per_sample"].get("ddpm_temb_batch_kernel")
    res = {
        "shape": {"ch": cfg.ch, "ch_mult": list(cfg.ch_mult), "attn_resolutions": list(cfg.attn_resolutions), "resolution": R,
                  "self_cond": True, "batch": B, "temb_rows": plan.temb_row_count},
        "device": torch.cuda.get_device_name(0),
        "forward_sc": stats(a), "forward_sc_again": stats(c), "forward_t": stats(b),
        "scalar_spread_ms": abs(statistics.median(a) - statistics.median(c)) + max(statistics.pstdev(a), statistics.pstdev(c)),
        "difference_ms": statistics.median(b) - statistics.median(a + c),
        "ddpm_temb_batch_kernel_ms": temb_ms,
        "kernel_rows_ms_per_launch": rows["per_sample"],
    }
    res["difference_minus_kernel_ms"] = res["difference_ms"] - (temb_ms or 0.0)
    res["accounted_for"] = abs(res["difference_minus_kernel_ms"]) <= res["scalar_spread_ms"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in res.items() if k != "kernel_rows_ms_per_launch"}))


if __name__ == "__main__":
    main()
