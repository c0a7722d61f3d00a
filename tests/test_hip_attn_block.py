"""attn_block64_kernel (csrc/attn_fused.hip: GroupNorm + qkv + softmax attention + proj + residual + the GroupNorm records of z
for an 8 x 8 x 64 block, one launch) through its own entry, mcedm_op_attn_block64, against the fp64 evaluation of
z = conv2d(attention(conv2d(group_norm(y)))) + y with the oracle's functions, at the project's bar (rtol 1e-4, atol 1e-5).

The network tests reach this kernel with uniform attention (|s| <= 0.02) that is 6 % of z; the cases of tests/_attn_block.py
are peaked (largest |score| 10 to 356, the running maximum in either key block and half-wave), overflow exp without the merged
maximum, put the probability mass on single keys, and give the register GroupNorm means of 600 standard deviations (under a large
residual, and under one small enough that a one-pass variance shows), group means of both signs and a zero variance.
tests/test_attn_block_cpu.py holds the cases to those regimes and the fp32 reference to the bar.

Worst error / bar measured on the MI355X: see DESIGN.md section 4, "The fused 8 x 8 attention block at kernel level"."""
import functools

import pytest
import torch

from oracle import fixtures as fx
from oracle import mcedm_oracle as orc
from tests import _attn_block as AB
from tests._attn_block import dev
from tests.test_hip_parity import close, lib, make_plan  # noqa: F401  (lib: fixture)

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def reference(name, B=3, tag="y"):
    """(parameters, y, fp64 z) of a case: computed once, shared, never written to."""
    P, y = AB.case(name, B, tag)
    return P, y, AB.tail64(P, y)


def held(got, ref, what):
    print(f"{what}: worst error / bar {AB.worst(got, ref):.3f}")
    close(got, ref, what=what)


@pytest.mark.parametrize("name", list(AB.CASES))
def test_attn_block_vs_fp64(lib, name):
    P, y, z64 = reference(name)
    z = lib.op_attn_block(dev(y), *AB.pack(lib, P))
    assert bool(torch.isfinite(z).all()), name
    held(z, z64, f"attn_block {name}")


def test_attn_block_batch_sizes_and_sample_independence(lib):
    """B = 1, 2, 5 on the peak40 parameters: one workgroup per sample, so a sample's bits do not depend on its batch."""
    P, y, z64 = reference("peak40", 5, "yB")
    args = AB.pack(lib, P)
    yd = dev(y)
    z5 = lib.op_attn_block(yd, *args)
    for B in (1, 2, 5):
        zB = lib.op_attn_block(yd[:B].contiguous(), *args)
        held(zB, z64[:B], f"attn_block peak40 B={B}")
        assert torch.equal(zB, z5[:B])
    for i in range(5):
        assert torch.equal(lib.op_attn_block(yd[i:i + 1].contiguous(), *args)[0], z5[i]), f"sample {i} alone"
    assert torch.equal(lib.op_attn_block(yd, *args), z5), "a repeated call"


@pytest.mark.parametrize("name", ["plain", "peak40", "mean300", "groups160", "tight"])
def test_attn_block_statistics_records(lib, name):
    """The (sum, M2) records of z per sample and 4-channel group -- what the next block's conv0 normalises with -- give the fp64
    mean and rstd of the fp64 z at the bar test_gn_coef_golden holds op_gn_coef to; asking for them does not change z."""
    P, y, z64 = reference(name)
    args = AB.pack(lib, P)
    z, gsum = lib.op_attn_block(dev(y), *args, want_sums=True)
    assert tuple(gsum.shape) == (3, 16, 2)
    assert torch.equal(z, lib.op_attn_block(dev(y), *args)), "z with and without the records"
    held(z, z64, f"attn_block {name} (with records)")
    mean64, rstd64 = AB.group_stats64(z64)
    g = gsum.double().cpu()
    held(g[..., 0] / 256, mean64, f"attn_block {name} group mean of z")
    held(1 / (g[..., 1] / 256 + 1e-5).sqrt(), rstd64, f"attn_block {name} group rstd of z")


@pytest.mark.parametrize("name", ["plain", "peak40", "diag"])
def test_attn_block_vs_three_launches(lib, name):
    P, y, z64 = reference(name)
    args = AB.pack(lib, P)
    z1 = lib.op_attn_block(dev(y), *args)
    z3 = AB.three_launches(lib, dev(y), *args)
    held(z1, z64, f"{name}: fused block vs fp64")
    held(z3, z64, f"{name}: three launches vs fp64")
    held(z1, z3.cpu(), f"{name}: fused block vs three launches")


@pytest.mark.parametrize("tag", ["attn", "catattn"])
@pytest.mark.parametrize("n_emb", [1, 2])
def test_unet_block_golden_with_fused_attention(lib, golden, tag, n_emb):
    """test_unet_block_golden with the attention tail of hip_block on the fused kernel: the reference's own block outputs."""
    x, emb = fx.block_inputs(tag, n_emb)
    y = AB.hip_block(lib, fx.block_params(tag), fx.block_spec(tag), x, emb, fused_attn=True)
    held(y, golden("blocks.npz")[f"{tag}_n{n_emb}_y"], f"block {tag} n_emb={n_emb}, fused attention")


def profiled(lib, fn):
    lib.prof_enable(True)
    try:
        fn()
        torch.cuda.synchronize()
        return {r["name"]: r["launches"] for r in lib.prof_report()}
    finally:
        lib.prof_enable(False)


def test_plan_dispatch_of_the_fused_block(lib):
    """Which forwards run the kernel: inference with the attention level at 8 x 8, once per attention block; no other."""
    plan = make_plan(lib, fx.CFG_P)
    packed = plan.pack({k: dev(v) for k, v in orc.make_params(fx.CFG_P, 7).items()})
    lab = dev(torch.tensor([0.4]))

    def forward(H, W, **kw):
        x, cond = dev(fx.randn("t/ab/disp/x", 2, 2, H, W)), dev(fx.randn("t/ab/disp/c", 2, 2, H, W))
        return profiled(lib, lambda: plan.forward(packed, x, lab, cond=cond, **kw))

    n_attn = sum(1 for n in plan.param_names if n.endswith(".qkv.weight"))
    assert n_attn == 4
    rows = forward(32, 32)
    assert rows.get("attn_block64_kernel") == n_attn and "attention_kernel" not in rows, rows
    rows = forward(40, 24)                    # attention at 10 x 6
    assert "attn_block64_kernel" not in rows and any(n.startswith("attention") for n in rows), rows
    rows = forward(32, 32, training=True)     # the backward needs qkv and the attention output
    assert "attn_block64_kernel" not in rows and any(n.startswith("attention") for n in rows), rows


def test_attn_block_bad_arguments_are_rejected_on_host(lib):
    P, y, _ = reference("plain")
    args = AB.pack(lib, P)
    yd, z = dev(y), torch.empty(3, 64, 8, 8, device="cuda")
    lb = lib._bind_ops()
    p = lib._ptr

    def call(y_ptr, B):
        gamma, beta, wq, bq, wp, bp = args
        lib.check(lb.mcedm_op_attn_block64(y_ptr, p(gamma), p(beta), 1e-5, p(wq), p(bq), p(wp), p(bp), p(z), None, B, lib._stream()))

    def rejected(y_ptr, B, match):
        with pytest.raises(RuntimeError, match=match):
            call(y_ptr, B)

    rows = profiled(lib, lambda: (rejected(None, 3, "null pointer"), rejected(p(yd), 0, "B = 0"), rejected(p(yd), -2, "B = -2")))
    assert "attn_block64_kernel" not in rows, rows
    with pytest.raises(RuntimeError, match=r"\[B, 64, 8, 8\]"):
        lib.op_attn_block(torch.zeros(2, 64, 8, 4, device="cuda"), *args)
    rows = profiled(lib, lambda: call(p(yd), 3))       # the same call with good arguments launches
    assert rows.get("attn_block64_kernel") == 1, rows
