"""GPU: the ADM U-Net executor (csrc/plan.hip, backward.hip) on every architecture of tests/_adm_arch.py -- widths 24 to 256, one
to five levels, one to three blocks per level, rectangular and ragged images, 1 to 3 state channels with and without
conditioning -- in inference AND through the training step, against the reference's own numbers (tests/golden/adm_arch.npz,
tools/make_golden_adm_arch.py) and against the fp64 evaluation of the same formulas, both at the project's bar (rtol 1e-4,
atol 1e-5 max|ref| per tensor), with proof from the profiler rows that the intended kernels ran (tests/_adm_arch.py PATHS), batch
independence, repeatability, and each kernel family switched off on the plan alone.

Worst err / bar per row (<= 1 passes).  CPU: the reference's own fp32 against fp64, as the generator prints it.  GPU: as these
tests print it on an MI355X, "vs the reference's run | vs fp64"; forward = the worst of the row's stored runs (D and F); the
gradient against the reference's run is the worst of the three stored tensors, against fp64 the worst of all parameters (named).

    row     CPU forward  loss    gradient                                 GPU forward       loss             gradient
    one     0.0357       0.0002  0.0811 dec.8x8_in0.norm0.weight          0.0639 | 0.0481   0.0000 | 0.0002  0.0682 | 0.1298 map_layer0.weight
    rect    0.0736       0.0010  0.3756 enc.32x32_conv.weight             0.2267 | 0.1888   0.0000 | 0.0010  0.1378 | 0.7137 enc.16x16_block0.norm0.weight
    ragged  0.0537       0.0005  0.4246 dec.3x3_in0.norm2.bias            0.1610 | 0.1290   0.0000 | 0.0005  0.5233 | 0.5466 enc.3x3_down.conv0.weight
    narrow  0.0653       0.0009  0.1833 dec.8x8_in0.conv0.weight          0.1359 | 0.1132   0.0000 | 0.0009  0.2393 | 0.4180 dec.8x8_in0.norm0.bias
    ch24    0.0523       0.0004  0.1992 enc.4x4_down.norm0.weight         0.1569 | 0.1277   0.0013 | 0.0009  0.1077 | 0.4212 enc.4x4_down.norm0.weight
    wide3   0.0721       0.0001  0.2548 dec.16x16_in1.norm1.weight        0.1390 | 0.1511   0.0007 | 0.0006  0.1961 | 0.5827 enc.16x16_block0.norm1.weight
    deep    0.1048       0.0001  0.3127 dec.2x2_in0.norm2.bias            0.1885 | 0.1094   0.0008 | 0.0008  0.3005 | 0.7549 enc.16x16_block0.norm0.bias
    nrb3    0.0440       0.0003  0.2782 dec.8x8_in0.norm2.weight          0.1046 | 0.0969   0.0000 | 0.0003  0.3297 | 0.9793 dec.8x8_in0.norm2.weight
    c192    0.0421       0.0001  0.0702 enc.32x32_conv.weight             0.0902 | 0.0736   0.0000 | 0.0001  0.0238 | 0.0881 enc.32x32_conv.weight
    c128a   0.0560       0.0004  0.1255 dec.16x16_in0.norm0.weight        0.1216 | 0.1035   0.0000 | 0.0004  0.0718 | 0.2422 dec.16x16_in1.conv0.weight
    attn_rag 0.0578      0.0005  0.2145 enc.20x20_block0.conv1.weight    0.1638 | 0.1919   0.0000 | 0.0005  0.2449 | 0.3641 enc.10x10_block0.conv1.weight

In the training step every row's attention_bwd_* profiler rows are those tests/_attn_bwd.py branch() predicts from its token counts:
the LDS kernels at 128, 256, 384, 512 and 1024 tokens, direct<1> at 4, 15, 16, direct<2> at 64 and (attn_rag) 100, direct<4> at 400.

With a kernel family switched off the forward stays below 0.22 | 0.19 (rect, conv_wino = 0) and the gradients where they were.
"""
import collections
import functools
import math

import pytest
import torch

from tests import _adm_arch as A
from tests import _attn_bwd as AB
from tests import _knobs as K

pytestmark = pytest.mark.gpu


def dev(t):
    return None if t is None else t.detach().contiguous().cuda()


@functools.lru_cache(maxsize=None)
def reference64(tag):
    """key -> (D, F) of the fp64 oracle, computed once per row."""
    P64 = A.params(tag, torch.float64)
    return {key: A.denoise_ref(tag, P64, kind) for key, kind in A.runs(tag)}


@functools.lru_cache(maxsize=None)
def training64(tag):
    """(loss, name -> gradient) by fp64 autograd through the oracle, computed once per row."""
    return A.training_grads(tag)


def build(tag, **variants):
    import mcedm_amd  # noqa: F401
    from mcedm_amd import lib as L
    assert torch.cuda.is_available()
    cfg = A.cfg_of(tag)
    plan = A.make_plan(L, cfg)
    for which, value in variants.items():      # before the first use: conv_wino shapes the workspace
        plan.set_variant(which, value)
    assert plan.param_names == [n for n, _ in A.orc.param_shapes(cfg)]
    params = {k: dev(v) for k, v in A.params(tag).items()}
    return L, plan, params, plan.pack(params)


@functools.lru_cache(maxsize=None)
def net(tag):
    return build(tag)


def infer(tag, plan, packed, kind, ws=None, sample=None):
    """One stored run -> (D, F) on the device (D None where the run has none); sample: that sample alone, as a batch of one."""
    sel = (lambda v: v) if sample is None else (lambda v: v[sample:sample + 1])
    I = A.inputs(tag)
    x, cond = dev(sel(I["x"])), None if I["cond"] is None else dev(sel(I["cond"]))
    if kind != "sigma":
        return None, plan.forward(packed, x, torch.tensor([A.LABEL]).cuda(), cond=cond if kind == "label" else None, ws=ws)
    if tag in A.PLAIN:
        return None, plan.forward(packed, x, dev(sel(A.plain_labels(tag))), cond=cond, ws=ws)
    return plan.denoise(packed, x, dev(sel(I["sigma"])), cond=cond, ws=ws, want_F=True)


def training_step(tag, L, plan, params, packed):
    """forward(training) -> loss -> backward into NaN-filled gradients; returns (loss [1], name -> gradient)."""
    I = {k: dev(v) for k, v in A.inputs(tag).items()}
    ws = L.Workspace()
    grads = [torch.full_like(params[n], float("nan")) for n in plan.param_names]
    if tag in A.PLAIN:
        labels, w = dev(A.plain_labels(tag)), dev(A.loss_weights(tag))
        F = plan.forward(packed, I["x"], labels, cond=I["cond"], ws=ws, training=True)
        loss = (w.double() * F.double() ** 2).sum().reshape(1)
        plan.unet_backward(packed, params, I["x"], labels, I["cond"], (2 * w * F).contiguous(), grads, ws)
    else:
        x_noise, sigma = L.edm_noise_inputs(I["x"], I["mask"], I["noise"], I["rnd_normal"].flatten())
        D = plan.denoise(packed, x_noise, sigma, cond=I["cond"], ws=ws, training=True)
        loss, dD = L.edm_loss(D, I["x"], I["mask"], sigma)
        plan.denoise_backward(packed, params, x_noise, sigma, I["cond"], dD, grads, ws)
    return loss, dict(zip(plan.param_names, grads))


def profiled(L, fn):
    """fn() with the profiler on -> (its result, kernel name -> launches; .variants: kernel name -> {variant: launches} for the
    rows whose launches name the kernel or instantiation they took)."""
    torch.cuda.synchronize()
    L.prof_enable(True)
    try:
        out = fn()
        torch.cuda.synchronize()
        report = L.prof_report()
    finally:
        L.prof_enable(False)
    rows = Rows((r["name"], int(r["launches"])) for r in report)
    rows.variants = {r["name"]: r["variants"] for r in report if r.get("variants")}
    return out, rows


class Rows(dict):
    variants = None


def fwd_variants(tag):
    """One launch_attention per attention block, on the kernel its token count selects (tests/_knobs.py attn_fwd_variant; the
    workspace is 16-byte aligned): variant -> launches."""
    return dict(collections.Counter(K.attn_fwd_variant(T) for T in A.attention_tokens(tag)))


def count(rows, prefix):
    return sum(v for k, v in rows.items() if k.startswith(prefix))


def golden_D(tag, F):
    """The denoiser output the reference's F gives: c_skip x + c_out F in fp64."""
    I = A.inputs(tag)
    c_skip, c_out, _, _ = A.orc.precond_coeffs(I["sigma"].double().reshape(-1, 1, 1, 1))
    return c_skip * I["x"].double() + c_out * torch.as_tensor(F).double()


def held_forward(tag, key, got, g, what=""):
    """(D, F) of one run against the golden and against the fp64 oracle, each at the bar; prints both ratios."""
    D, F = got
    D64, F64 = reference64(tag)[key]
    assert F.dtype == torch.float32 and bool(torch.isfinite(F).all())
    rg, r64 = A.bar_ratio(F, g[key]), A.bar_ratio(F, F64)
    if D is not None:
        assert bool(torch.isfinite(D).all())
        rg, r64 = max(rg, A.bar_ratio(D, golden_D(tag, g[key]))), max(r64, A.bar_ratio(D, D64))
    print(f"{key}{what}: worst err / bar {rg:.4f} vs the reference's run, {r64:.4f} vs the fp64 oracle")
    assert rg <= 1.0 and r64 <= 1.0, (key, what, rg, r64)


def held_training(tag, loss, grads, g, what=""):
    """Loss and EVERY parameter gradient against fp64 autograd; the loss, the per-parameter gradient norms and the three stored
    gradients against the reference network's own autograd; all at the bar.  Prints the worst of each."""
    loss64, g64 = training64(tag)
    assert all(bool(torch.isfinite(v).all()) for v in grads.values()), [n for n, v in grads.items() if not bool(torch.isfinite(v).all())]
    rl64, rlg = A.bar_ratio(loss, loss64.reshape(1)), A.bar_ratio(loss, g[f"{tag}::loss"].reshape(1))
    r64, n64 = max((A.bar_ratio(grads[n], g64[n]), n) for n in grads)
    rg, ng = max((A.bar_ratio(grads[n], g[f"{tag}::grad::{n}"]), n) for n in A.grad_names(tag))
    norms = torch.tensor([math.sqrt(float((v.double() ** 2).sum())) for v in grads.values()], dtype=torch.float64)
    rn = A.bar_ratio(norms, torch.as_tensor(g[f"{tag}::grad_sqnorm_each"]).sqrt())
    print(f"{tag}{what}: worst err / bar: loss {rlg:.4f} vs the reference's run, {rl64:.4f} vs fp64; gradients {r64:.4f} vs fp64 ({n64}), "
          f"{rg:.4f} vs the reference's run ({ng}), gradient norms {rn:.4f} vs the reference's run")
    assert max(rl64, rlg, r64, rg, rn) <= 1.0, (tag, what, rl64, rlg, (r64, n64), (rg, ng), rn)


# ---- 1. inference: every row against the reference and the fp64 oracle --------------------------------------------------------------
@pytest.mark.parametrize("tag", list(A.ARCHS))
def test_inference_golden_and_fp64(golden, tag):
    """denoise at one noise level per sample (0.05 to 30), forward at one broadcast label, and cond = None where the row has
    conditioning channels."""
    g = golden("adm_arch.npz")
    L, plan, params, packed = net(tag)
    for key, kind in A.runs(tag):
        held_forward(tag, key, infer(tag, plan, packed, kind), g)


# ---- 2. the training step ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", list(A.ARCHS))
def test_training_step_golden_and_fp64(golden, tag):
    """forward(training) -> loss -> backward; gradients pre-filled with NaN; a second step gives the same bits.  What the backward
    is expected to launch: one attention_kernel per attention block (the fused 8 x 8 block is inference only), one attention_bwd_*
    row per block on the branch tests/_attn_bwd.py branch() predicts from its token count, no split Winograd
    kernel (AdmNet::conv: training carries no Winograd table below 32 x 32), the thin weight-gradient kernels of the plain row."""
    g = golden("adm_arch.npz")
    L, plan, params, packed = net(tag)
    (loss, grads), rows = profiled(L, lambda: training_step(tag, L, plan, params, packed))
    held_training(tag, loss, grads, g)
    loss2, grads2 = training_step(tag, L, plan, params, packed)
    assert torch.equal(loss, loss2) and all(torch.equal(grads[n], grads2[n]) for n in grads)
    assert count(rows, "attn_block64") == 0 and rows.get("attention_kernel", 0) == len(A.attention_tokens(tag)), rows
    assert rows.variants.get("attention_kernel", {}) == fwd_variants(tag), (rows.variants, fwd_variants(tag))
    # the attention backward, one launch per block on the branch its token count selects (the workspace is 16-byte aligned)
    want = collections.Counter("attention_bwd_" + AB.branch(T) for T in A.attention_tokens(tag))
    assert {k: v for k, v in rows.items() if k.startswith("attention_bwd")} == dict(want), (rows, want)
    if tag == "attn_rag":
        assert want == {"attention_bwd_direct<4>": 3, "attention_bwd_direct<2>": 4}
    assert count(rows, "conv_wino_kernel<WinoSplitCfg") == 0 and count(rows, "conv_wino_kernel<WinoSkipCfg") == 0, sorted(rows)
    if tag in A.THIN_WGRADS:
        assert count(rows, "wgrad_thin_kernel") + count(rows, "wgrad_thin4_kernel") == A.THIN_WGRADS[tag], rows
    if tag in A.WGRAD_WINO:
        assert rows.get("wgrad_wino_kernel", 0) > 0, sorted(rows)


# ---- 3. the intended path ran ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", list(A.ARCHS))
def test_the_intended_kernels_ran(tag):
    """The profiler rows of one inference call against tests/_adm_arch.py PATHS (each entry justified there by its predicate)."""
    L, plan, params, packed = net(tag)
    infer(tag, plan, packed, "sigma")            # anything lazily initialised settles outside the recording
    _, rows = profiled(L, lambda: infer(tag, plan, packed, "sigma"))
    want = A.PATHS[tag]
    got = dict(wino=count(rows, "conv_wino_kernel<WinoCfg") + count(rows, "conv_wino_kernel<WinoSkipCfg") + count(rows, "conv_wino1") > 0,
               split=count(rows, "conv_wino_kernel<WinoSplitCfg") > 0, fold=count(rows, "conv_wino_kernel<WinoSkipCfg") > 0,
               table=rows.get("gn_coef_kernel", 0) > 0)
    assert got == want, (tag, got, want, sorted(rows))
    if not want["wino"] and not want["split"]:
        assert count(rows, "conv_wino") == 0, sorted(rows)
    n_attn = len(A.attention_tokens(tag))
    if tag in A.FUSED_ATTN:
        assert count(rows, "attn_block64") == n_attn == 4 and rows.get("attention_kernel", 0) == 0, rows
    else:
        assert count(rows, "attn_block64") == 0 and rows.get("attention_kernel", 0) == n_attn, rows
        assert rows.variants.get("attention_kernel", {}) == fwd_variants(tag), (rows.variants, fwd_variants(tag))


# ---- 4. batch independence, repeatability -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", list(A.ARCHS))
def test_sample_alone_and_second_call_are_bit_identical(tag):
    """Sample B - 1 of the batched call == the B = 1 call on that sample (every kernel is chosen by shape alone, never by the batch
    size, and no sum's order depends on it); a second call on the same workspace == the first."""
    L, plan, params, packed = net(tag)
    B = A.ARCHS[tag][1]
    ws = L.Workspace()
    first = [None if v is None else v.clone() for v in infer(tag, plan, packed, "sigma", ws=ws)]
    again = infer(tag, plan, packed, "sigma", ws=ws)
    alone = infer(tag, plan, packed, "sigma", sample=B - 1)
    for a, b, c in zip(first, again, alone):
        if a is not None:
            assert torch.equal(a, b), float((a - b).abs().max())
            assert torch.equal(c[0], a[B - 1]), float((c[0] - a[B - 1]).abs().max())


# ---- 5. kernel families switched off on this plan alone ---------------------------------------------------------------------------------
@pytest.mark.parametrize("which,tag", [(w, t) for w, (tags, _) in A.SWITCHED.items() for t in tags])
def test_kernel_family_switched_off_stays_within_the_bar(golden, which, tag):
    g = golden("adm_arch.npz")
    L, plan, params, packed = build(tag, **{which: 0})
    got, rows = profiled(L, lambda: infer(tag, plan, packed, "sigma"))
    assert count(rows, A.SWITCHED[which][1]) == 0, sorted(rows)
    held_forward(tag, f"{tag}::F_sigma", got, g, what=f" [{which} = 0]")
    if which == "attn_fused":
        assert rows.get("attention_kernel", 0) == len(A.attention_tokens(tag)), rows
        assert rows.variants.get("attention_kernel", {}) == fwd_variants(tag), (rows.variants, fwd_variants(tag))
    if which == "conv_wino_fold":
        # the projections the fold served run as their own launches: try_launch_conv1x1_reg (128 output channels, 1024 pixels)
        assert rows.get("conv1x1_reg_kernel", 0) > 0, sorted(rows)
        assert rows.variants["conv1x1_reg_kernel"] == {"<2, 128>": rows["conv1x1_reg_kernel"]}, rows.variants


def test_fold_and_register_gemm_both_off(golden):
    """c128a with the fold off is where conv1x1_reg_kernel is in play in inference (try_launch_conv1x1_reg: 64-channel projections
    need 4096 pixels, which no row has); with both off the projections fall to the resident / tiled 1x1 kernels."""
    g = golden("adm_arch.npz")
    L, plan, params, packed = build("c128a", conv_wino_fold=0, conv1x1_reg=0)
    got, rows = profiled(L, lambda: infer("c128a", plan, packed, "sigma"))
    assert count(rows, "conv1x1_reg") == 0 and count(rows, "conv_wino_kernel<WinoSkipCfg") == 0, sorted(rows)
    held_forward("c128a", "c128a::F_sigma", got, g, what=" [conv_wino_fold = 0, conv1x1_reg = 0]")


@pytest.mark.parametrize("which,tag", [(w, t) for w, (tags, _) in A.SWITCHED_TRAINING.items() for t in tags])
def test_kernel_family_switched_off_in_the_training_step(golden, which, tag):
    g = golden("adm_arch.npz")
    L, plan, params, packed = build(tag, **{which: 0})
    (loss, grads), rows = profiled(L, lambda: training_step(tag, L, plan, params, packed))
    assert count(rows, A.SWITCHED_TRAINING[which][1]) == 0, sorted(rows)
    held_training(tag, loss, grads, g, what=f" [{which} = 0]")
