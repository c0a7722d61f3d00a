"""Device time of SweFvLoss.unroll_from_init: the fused unroll (mcedm_swe_fv_unroll, one launch) against the only other route to
the same tensor, a loop of n_steps f_t_swp1d calls plus torch.cat, at the reference's evaluation shape (n_samples 5 x batch 32
states of 128 x 128).  Device events around repeated calls, five alternated rounds in one process; the two results are compared
bit for bit before anything is timed.

    python tools/swe_unroll_bench.py [--rounds 5] [--out profiles/swe_unroll_bench.json]

Exits non-zero if the fused call is not the faster one in every round.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mcedm_amd  # noqa: F401,E402
from mcedm_amd import pde_loss  # noqa: E402
from tests import _swe_unroll as U  # noqa: E402


def device_ms(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=160)
    ap.add_argument("--steps", type=int, default=127)
    ap.add_argument("--x", type=int, default=128)
    ap.add_argument("--system", default="swe", choices=list(U.SYSTEMS))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps-fused", type=int, default=400)
    ap.add_argument("--reps-loop", type=int, default=40)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "swe_unroll_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark measures the GPU; there is nothing to fall back to"
    f = pde_loss.SweFvLoss(**U.SYSTEMS[a.system])
    ic = U.initial_condition("bench", a.batch, a.x).cuda()

    def fused():
        return f.unroll_from_init(ic, a.steps)

    def loop():
        rows, cur = [ic], ic
        for _ in range(a.steps):
            cur = f.f_t_swp1d(cur, f.Tn / a.steps)
            rows.append(cur)
        return torch.cat(rows, dim=1)

    # the C entry alone into a preallocated buffer: what is left of `fused` without the drop-in's host work (gen_x, allocation)
    import numpy as np
    from mcedm_amd import lib as L
    out = torch.empty(a.batch, a.steps + 1, a.x, 2, device="cuda")
    half_dt, dx, entry = float(np.float32(0.5 * (f.Tn / a.steps))), f._dx(a.x), L.load().mcedm_swe_fv_unroll
    stream = torch.cuda.current_stream().cuda_stream

    def c_call():
        L.check(entry(ic.data_ptr(), 2 * a.x, out.data_ptr(), None, None, a.batch, a.steps, a.x, half_dt, dx, 1.0, 1.0, stream))

    got, want = fused(), loop()
    c_call()
    assert bool(torch.isfinite(want).all()) and torch.equal(got, want) and torch.equal(out, want), "the fused unroll differs from the loop"
    for fn in (fused, loop, c_call):              # warm all before the first timed window
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    rounds = []
    for r in range(a.rounds):
        t_fused = device_ms(fused, a.reps_fused)
        t_loop = device_ms(loop, a.reps_loop)
        t_c = device_ms(c_call, a.reps_fused)
        rounds.append({"fused_ms": t_fused, "loop_ms": t_loop, "loop_over_fused": t_loop / t_fused, "c_call_ms": t_c})
        print(f"round {r}: fused {t_fused * 1e3:9.1f} us   loop of {a.steps} steps + cat {t_loop * 1e3:9.1f} us   ratio {t_loop / t_fused:7.1f}"
              f"   C entry alone {t_c * 1e3:9.1f} us")
    med = lambda k: sorted(x[k] for x in rounds)[len(rounds) // 2]
    cells = a.batch * a.steps * a.x
    res = {"bench": "swe_unroll", "device": torch.cuda.get_device_name(0), "system": a.system, "B": a.batch, "T": a.steps + 1,
           "X": a.x, "n_steps": a.steps, "reps_fused": a.reps_fused, "reps_loop": a.reps_loop, "timing": "device events, per call",
           "bit_identical": True, "rounds": rounds, "fused_ms_median": med("fused_ms"), "loop_ms_median": med("loop_ms"),
           "loop_over_fused_median": med("loop_over_fused"), "c_call_ms_median": med("c_call_ms"),
           "loop_us_per_step_median": med("loop_ms") * 1e3 / a.steps,
           "c_call_ns_per_step_median": med("c_call_ms") * 1e6 / a.steps, "c_call_gcell_per_s_median": cells / med("c_call_ms") / 1e6,
           "fused_faster_in_every_round": all(x["fused_ms"] < x["loop_ms"] for x in rounds)}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps({k: v for k, v in res.items() if k != "rounds"}))
    if not res["fused_faster_in_every_round"]:
        raise SystemExit("the fused unroll was not faster than the loop in every round")


if __name__ == "__main__":
    main()
