"""GPU: dropout in the ADM U-Net's training step (include/mcedm_hip.h mcedm_unet_plan_set_dropout; csrc/edm.hip dropout_act_kernel /
dropout_scale_kernel; plan.hip run_block; backward.hip block_backward).  Every comparison is against a deterministic reference:
the masks are what mcedm_uniform_fill writes, bit for bit, and the numbers are the fp64 oracle's with those masks injected
(tests/_adm_dropout.py) and the reference's own run (tests/golden/adm_dropout.npz).

Worst err / bar (rtol 1e-4, atol 1e-5 max|ref|; <= 1 passes) of the training step at p = 0.25 as test_training_step_with_dropout
prints it on an MI355X, beside the same rows at p = 0 (tests/test_hip_adm_arch.py): see DESIGN.md section 7c.

PARENT_ROWS: the profiler rows (kernel name -> launches) of the p = 0 training step of each row as the commit BEFORE dropout
launched them, recorded once on an MI355X with that commit's library; test_p0_launches_what_the_parent_launched holds this commit
to them.
"""
import functools
import math

import numpy as np
import pytest
import torch

from oracle import fixtures as fx
from oracle import mcedm_oracle as orc
from tests import _adm_arch as A
from tests import _adm_dropout as D
from tests.test_hip_adm_arch import build, count, dev, profiled

pytestmark = pytest.mark.gpu

P = D.P_DROP
SEED = D.SEED
PARENT_ROWS = {
    'narrow': {
        'act_materialize_kernel': 3,
        'conv_mfma_kernel<ConvCfg<32, 8, 8, 1, 2, 1, 16, 256, 1>, 0>': 3,
        'conv_mfma_kernel<ConvCfg<32, 8, 8, 1, 2, 9, 8, 256, 1>, 0>': 14,
        'conv_mfma_kernel<ConvCfg<64, 8, 8, 2, 2, 9, 8, 256, 1>, 0>': 1,
        'conv_resident_kernel<ResCfg<32, 4, 8, 1, 1, 9, 8, 4>, 0, false>': 23,
        'conv_resident_kernel<ResCfg<64, 8, 8, 2, 2, 1, 16, 1>, 0, false>': 2,
        'conv_resident_kernel<ResCfg<64, 8, 8, 2, 2, 9, 8, 1>, 0, false>': 4,
        'conv_resident_kernel<ResCfg<64, 8, 8, 2, 2, 9, 8, 1>, 1, false>': 1,
        'gn_bwd_kernel': 2,
        'gn_bwd_reg_kernel': 19,
        'gn_coef_from_sums_kernel': 20,
        'gn_coef_kernel': 1,
        'wgrad_kernel<WgCfg<4, 16, 1>>': 2,
        'wgrad_kernel<WgCfg<4, 16, 9>>': 8,
        'wgrad_kernel<WgCfg<8, 8, 1>>': 3,
        'wgrad_kernel<WgCfg<8, 8, 9>>': 12,
        'wgrad_reduce_kernel': 25,
        'wgrad_thin4_kernel': 2,
    },
    'ragged': {
        'act_materialize_kernel': 6,
        'attention_bwd_direct<1>': 4,
        'attention_kernel': 4,
        'conv_mfma_kernel<ConvCfg<32, 8, 8, 1, 2, 9, 8, 256, 1>, 0>': 1,
        'conv_resident_kernel<ResCfg<32, 4, 8, 1, 1, 9, 8, 4>, 0, false>': 24,
        'conv_resident_kernel<ResCfg<64, 8, 8, 2, 2, 1, 16, 1>, 0, false>': 23,
        'conv_resident_kernel<ResCfg<64, 8, 8, 2, 2, 9, 8, 1>, 0, false>': 36,
        'conv_resident_kernel<ResCfg<64, 8, 8, 2, 2, 9, 8, 1>, 1, false>': 2,
        'gn_bwd_kernel': 35,
        'gn_coef_from_sums_kernel': 33,
        'gn_coef_kernel': 2,
        'wgrad_kernel<WgCfg<4, 16, 1>>': 2,
        'wgrad_kernel<WgCfg<4, 16, 9>>': 8,
        'wgrad_kernel<WgCfg<8, 8, 1>>': 13,
        'wgrad_kernel<WgCfg<8, 8, 9>>': 22,
        'wgrad_reduce_kernel': 45,
        'wgrad_thin_kernel': 2,
    },
    'rect': {
        'act_materialize_kernel': 3,
        'attention_bwd_lds': 1,
        'attention_kernel': 1,
        'conv1x1_reg_kernel': 1,
        'conv_mfma_kernel<ConvCfg<32, 8, 32, 1, 4, 1, 16, 256, 1>, 0>': 3,
        'conv_mfma_kernel<ConvCfg<32, 8, 32, 1, 4, 9, 8, 256, 1>, 0>': 3,
        'conv_resident_kernel<ResCfg<64, 8, 16, 1, 4, 1, 16, 1>, 0, false>': 7,
        'conv_resident_kernel<ResCfg<64, 8, 16, 1, 4, 9, 8, 1>, 0, true>': 24,
        'conv_wino_kernel<WinoCfg<2>, false, false>': 5,
        'conv_wino_kernel<WinoCfg<2>, false, true>': 6,
        'conv_wino_kernel<WinoCfg<4>, false, false>': 3,
        'conv_wino_kernel<WinoCfg<4>, false, true>': 1,
        'conv_wino_kernel<WinoCfg<4>, true, true, WinoUp<true>>': 1,
        'gn_bwd_kernel': 15,
        'gn_bwd_reg_kernel': 7,
        'gn_coef_from_sums_kernel': 20,
        'gn_coef_kernel': 2,
        'wgrad_kernel<WgCfg<2, 32, 1>>': 7,
        'wgrad_kernel<WgCfg<2, 32, 9>>': 20,
        'wgrad_reduce_kernel': 27,
        'wgrad_thin_kernel': 2,
    },
    'c128a': {
        'act_materialize_kernel': 3,
        'attention_bwd_lds': 7,
        'attention_kernel': 7,
        'conv1x1_reg_kernel': 7,
        'conv_resident_kernel<ResCfg<32, 8, 16, 1, 4, 9, 8, 1>, 0, true>': 1,
        'conv_resident_kernel<ResCfg<64, 8, 16, 1, 4, 1, 16, 1>, 0, false>': 9,
        'conv_resident_kernel<ResCfg<64, 8, 16, 1, 4, 9, 8, 1>, 0, true>': 2,
        'conv_resident_kernel<ResCfg<64, 8, 8, 2, 2, 1, 16, 1>, 0, false>': 18,
        'conv_resident_kernel<ResCfg<64, 8, 8, 2, 2, 9, 8, 1>, 0, false>': 24,
        'conv_wino_kernel<WinoCfg<4>, false, false>': 8,
        'conv_wino_kernel<WinoCfg<4>, false, true>': 7,
        'conv_wino_kernel<WinoCfg<4>, true, true, WinoUp<true>>': 1,
        'gn_bwd_kernel': 2,
        'gn_bwd_reg_kernel': 26,
        'gn_coef_from_sums_kernel': 28,
        'wgrad_kernel<WgCfg<2, 32, 1>>': 8,
        'wgrad_kernel<WgCfg<4, 16, 1>>': 10,
        'wgrad_kernel<WgCfg<4, 16, 9>>': 12,
        'wgrad_reduce_kernel': 30,
        'wgrad_thin4_kernel': 2,
        'wgrad_wino_kernel': 8,
        'wgrad_wino_reduce_kernel': 8,
    },
    'ch24': {
        'act_materialize_kernel': 7,
        'conv_mfma_kernel<ConvCfg<32, 8, 32, 1, 4, 1, 16, 256, 1>, 0>': 1,
        'conv_mfma_kernel<ConvCfg<32, 8, 32, 1, 4, 9, 8, 256, 1>, 0>': 2,
        'conv_mfma_kernel<ConvCfg<32, 8, 8, 1, 2, 1, 16, 256, 1>, 0>': 5,
        'conv_mfma_kernel<ConvCfg<32, 8, 8, 1, 2, 9, 8, 256, 1>, 0>': 7,
        'conv_mfma_kernel<ConvCfg<64, 8, 8, 2, 2, 9, 8, 256, 1>, 0>': 2,
        'conv_resident_kernel<ResCfg<32, 4, 8, 1, 1, 9, 8, 4>, 0, false>': 24,
        'conv_resident_kernel<ResCfg<32, 8, 16, 1, 4, 9, 8, 1>, 0, true>': 12,
        'conv_resident_kernel<ResCfg<64, 8, 16, 1, 4, 1, 16, 1>, 0, false>': 1,
        'conv_resident_kernel<ResCfg<64, 8, 16, 1, 4, 9, 8, 1>, 0, true>': 4,
        'conv_resident_kernel<ResCfg<64, 8, 16, 1, 4, 9, 8, 1>, 1, true>': 1,
        'conv_resident_kernel<ResCfg<64, 8, 8, 2, 2, 9, 8, 1>, 0, false>': 10,
        'conv_resident_kernel<ResCfg<64, 8, 8, 2, 2, 9, 8, 1>, 1, false>': 1,
        'gn_bwd_kernel': 15,
        'gn_bwd_reg_kernel': 16,
        'gn_coef_from_sums_kernel': 31,
        'wgrad_kernel<WgCfg<2, 32, 1>>': 2,
        'wgrad_kernel<WgCfg<2, 32, 9>>': 9,
        'wgrad_kernel<WgCfg<4, 16, 1>>': 3,
        'wgrad_kernel<WgCfg<4, 16, 9>>': 10,
        'wgrad_kernel<WgCfg<8, 8, 1>>': 2,
        'wgrad_kernel<WgCfg<8, 8, 9>>': 12,
        'wgrad_reduce_kernel': 38,
        'wgrad_thin4_kernel': 1,
    },
}


def seed_tensor(v):
    return torch.tensor([v], dtype=torch.int64, device="cuda")


@functools.lru_cache(maxsize=None)
def net(tag):
    return build(tag)


def device_masks(L, tag, seed, p=P):
    cfg, B, H, W = A.ARCHS[tag]
    st = seed_tensor(seed)
    return D.masks_for(cfg, B, H, W, p, seed, keep=lambda j, shape: D.keep_device(L, st, j, shape, p))


@functools.lru_cache(maxsize=None)
def reference64(tag):
    """(loss, name -> gradient, F) of the fp64 oracle with the DEVICE generator's masks injected, once per row."""
    L = net(tag)[0]
    masks = device_masks(L, tag, SEED)
    loss, grads = D.training_grads(tag, masks)
    return loss, grads, D.forward_F(tag, masks)


def training_step(tag, L, plan, params, packed, ws=None, between=None):
    """forward(training) -> loss -> backward into NaN-filled gradients; between(): runs between the forward and the backward.
    Returns (loss [1], name -> gradient, F)."""
    I = {k: dev(v) for k, v in A.inputs(tag).items()}
    ws = ws or L.Workspace()
    grads = [torch.full_like(params[n], float("nan")) for n in plan.param_names]
    if tag in A.PLAIN:
        labels, w = dev(A.plain_labels(tag)), dev(A.loss_weights(tag))
        F = plan.forward(packed, I["x"], labels, cond=I["cond"], ws=ws, training=True)
        loss = (w.double() * F.double() ** 2).sum().reshape(1)
        if between:
            between()
        plan.unet_backward(packed, params, I["x"], labels, I["cond"], (2 * w * F).contiguous(), grads, ws)
    else:
        x_noise, sigma = L.edm_noise_inputs(I["x"], I["mask"], I["noise"], I["rnd_normal"].flatten())
        D_, F = plan.denoise(packed, x_noise, sigma, cond=I["cond"], ws=ws, training=True, want_F=True)
        loss, dD = L.edm_loss(D_, I["x"], I["mask"], sigma)
        if between:
            between()
        plan.denoise_backward(packed, params, x_noise, sigma, I["cond"], dD, grads, ws)
    return loss, dict(zip(plan.param_names, grads)), F


def same(a, b):
    return torch.equal(a[0], b[0]) and all(torch.equal(a[1][n], b[1][n]) for n in a[1])


# ---- 1. the two kernels alone ---------------------------------------------------------------------------------------------------------------
SHAPES = [(2, 64, 32, 32), (3, 40, 3, 5), (1, 8, 1, 1)]


def silu64(t):
    return t / (1 + torch.exp(-t))


@pytest.mark.parametrize("draw", [0, 7])
@pytest.mark.parametrize("p", [0.1, 0.5, 1e-6])
@pytest.mark.parametrize("shape", SHAPES)
def test_op_kernels(shape, p, draw):
    """dropout_act: the zero pattern is uniform_fill < p bit for bit, kept values are silu(coef h) / (1 - p) at the bar; per-sample
    rows, one broadcast row and no rows at all.  dropout_scale: the same pattern, g * s on the kept elements, in place.  16-byte
    body at 32 x 32, scalar path on 15- and 1-element planes (odd batch) and on a tensor one element off a 16-byte boundary."""
    L = net("narrow")[0]
    Bn, Cn, H, W = shape
    n = Bn * Cn * H * W
    st = seed_tensor(SEED)
    tagk = f"drop/{Bn}x{Cn}x{H}x{W}"
    h = fx.randn(tagk + "/h", *shape) * 2.0
    coef = torch.stack([fx.randn(tagk + "/mean", Bn, Cn) * 0.3, 0.5 + fx.randn(tagk + "/scale", Bn, Cn).abs(),
                        fx.randn(tagk + "/off", Bn, Cn) * 0.5, torch.zeros(Bn, Cn)], dim=-1).contiguous()
    u = L.uniform_fill(torch.empty(shape, device="cuda"), st, draw).cpu()
    p32 = float(np.float32(p))
    drop = u < p32
    s64 = 1.0 / (1.0 - p32)
    for rows, batch in ((coef, 1), (coef[:1].contiguous(), 0), (None, 1)):
        out = L.op_dropout_act(dev(h), p, st, draw, coef=dev(rows), coef_batch=batch).cpu()
        # (a kept silu(t) is zero only at t = 0 or below t = -88, which these inputs never reach: the zeros ARE the mask)
        assert torch.equal(out == 0, drop), "zero pattern != uniform_fill < p"
        c =torch.tensor([0.0, 1.0, 0.0, 0.0]).expand(Bn, Cn, 4) if rows is None else rows.expand(Bn, Cn, 4)
        c = c.double()[:, :, :, None, None]
        ref = silu64((h.double() - c[:, :, 0]) * c[:, :, 1] + c[:, :, 2]) * s64 * (~drop)
        assert A.bar_ratio(out, ref) <= 1.0, (shape, p, draw, batch, A.bar_ratio(out, ref))
    g = fx.randn(tagk + "/g", *shape)
    got = L.op_dropout_scale(dev(g).clone(), p, st, draw).cpu()
    assert torch.equal(got == 0, drop | (g == 0))
    assert A.bar_ratio(got, g.double() * s64 * (~drop)) <= 1.0
    # one element past a 16-byte boundary: the scalar path gives the same values (the mask depends on the element index alone)
    buf = torch.full((n + 2,), 7.0, device="cuda")
    buf[1:n + 1] = dev(g).flatten()
    view = buf[1:n + 1].view(shape)
    assert view.data_ptr() % 16 == 4
    L.op_dropout_scale(view, p, st, draw)
    assert torch.equal(view.cpu(), got) and float(buf[0]) == 7.0 and float(buf[n + 1]) == 7.0
    if shape == SHAPES[0] and p == 0.1:
        k = int(drop.sum())
        assert abs(k - n * p) <= 6 * math.sqrt(n * p * (1 - p)), (k, n * p)      # deterministic for the fixed seed


def test_op_kernels_reject_bad_probabilities():
    L = net("narrow")[0]
    st = seed_tensor(SEED)
    x = torch.zeros(1, 8, 4, 4, device="cuda")
    for p in (0.0, 1.0, -0.5, float("nan")):
        with pytest.raises(RuntimeError, match=r"\(0, 1\)"):
            L.op_dropout_act(x, p, st, 0)
        with pytest.raises(RuntimeError, match=r"\(0, 1\)"):
            L.op_dropout_scale(x, p, st, 0)


# ---- 2. the training step -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", D.ROWS)
def test_training_step_with_dropout(golden, tag):
    """p = 0.25: loss and EVERY parameter gradient against the fp64 oracle with the masks injected; narrow and rect also against the
    reference's own run; gradient buffers pre-filled with NaN; one dropout_act_kernel and one dropout_scale_kernel per block and no
    other row that the p = 0 step does not have."""
    L, plan, params, packed = build(tag)
    nblocks = len(D.block_shapes(*A.ARCHS[tag]))
    (loss0, _, F0), rows0 = profiled(L, lambda: training_step(tag, L, plan, params, packed))
    plan.set_dropout(P, seed_tensor(SEED))
    (loss, grads, F), rows = profiled(L, lambda: training_step(tag, L, plan, params, packed))
    assert all(bool(torch.isfinite(v).all()) for v in grads.values()), [n for n, v in grads.items() if not bool(torch.isfinite(v).all())]
    loss64, g64, F64 = reference64(tag)
    r_f, r_l = A.bar_ratio(F, F64), A.bar_ratio(loss, loss64.reshape(1))
    r_g, n_g = max((A.bar_ratio(grads[n], g64[n]), n) for n in grads)
    print(f"{tag} [dropout {P}]: worst err / bar vs the fp64 oracle with the same masks: F {r_f:.4f}, loss {r_l:.4f}, gradients {r_g:.4f} ({n_g})")
    assert max(r_f, r_l, r_g) <= 1.0, (tag, r_f, r_l, (r_g, n_g))
    assert A.bar_ratio(F, F0.cpu()) > 100.0                                     # and it is not the p = 0 step
    if tag in D.GOLDEN_ROWS:
        g = golden("adm_dropout.npz")
        assert int(g["seed"]) == SEED and float(g["p"]) == P
        rf, rl = A.bar_ratio(F, g[f"{tag}::F"]), A.bar_ratio(loss, g[f"{tag}::loss"].reshape(1))
        rg, ng = max((A.bar_ratio(grads[n], g[f"{tag}::grad::{n}"]), n) for n in D.golden_grad_names(tag))
        norms = torch.tensor([math.sqrt(float((v.double() ** 2).sum())) for v in grads.values()], dtype=torch.float64)
        rn = A.bar_ratio(norms, torch.as_tensor(g[f"{tag}::grad_sqnorm_each"]).sqrt())
        print(f"{tag} [dropout {P}]: worst err / bar vs the reference's run: F {rf:.4f}, loss {rl:.4f}, stored gradients {rg:.4f} ({ng}), "
              f"gradient norms {rn:.4f}")
        assert max(rf, rl, rg, rn) <= 1.0, (tag, rf, rl, (rg, ng), rn)
    assert rows.get("dropout_act_kernel", 0) == nblocks and rows.get("dropout_scale_kernel", 0) == nblocks, rows
    assert set(rows) - set(rows0) == {"dropout_act_kernel", "dropout_scale_kernel"}, sorted(set(rows) - set(rows0))
    assert count(rows0, "dropout") == 0


# ---- 3. seeds ---------------------------------------------------------------------------------------------------------------------------------
def saved_inputs(ws, tag, seed):
    """The per-block xd1 tensors out of the training workspace: they lie in block order right in front of the seed slot, which is
    found by its value (each 256-byte aligned, as mcedm_unet_workspace_bytes accounts for them)."""
    words = ws.buf[: ws.buf.numel() // 8 * 8].view(torch.int64)
    at = (words == seed).nonzero().flatten().tolist()
    assert len(at) == 1, at
    end = at[0] * 8
    out = {}
    for key, shape in reversed(D.block_shapes(*A.ARCHS[tag])):
        nbytes = 4 * math.prod(shape)
        end -= (nbytes + 255) // 256 * 256
        out[key] = ws.buf[end:end + nbytes].view(torch.float32).view(shape).cpu()
    return out


def test_seeds():
    tag = "narrow"
    L, plan, params, packed = build(tag)
    seed = seed_tensor(SEED)
    plan.set_dropout(P, seed)
    ws = L.Workspace()
    first = training_step(tag, L, plan, params, packed, ws=ws)
    # the materialised conv1 inputs: zero exactly where the device generator's draw j says so; blocks of equal shape differ
    xd1 = saved_inputs(ws, tag, SEED)
    masks = device_masks(L, tag, SEED)
    for key in masks:
        assert torch.equal(xd1[key] == 0, masks[key] == 0), key
    keys = list(masks)
    pairs = [(a, b) for i, a in enumerate(keys) for b in keys[i + 1:] if masks[a].shape == masks[b].shape]
    assert pairs and all(not torch.equal(xd1[a] == 0, xd1[b] == 0) for a, b in pairs)
    # same seed, second step: the same bits
    assert same(first, training_step(tag, L, plan, params, packed, ws=ws))
    # the host rewrites *rng_seed between the forward and the backward: the backward still regenerates the forward's masks
    disturbed = training_step(tag, L, plan, params, packed, ws=ws, between=lambda: seed.fill_(SEED + 12345))
    assert same(first, disturbed)
    assert int(seed.item()) == SEED + 12345
    # another seed: another network output
    other = training_step(tag, L, plan, params, packed, ws=ws)
    assert not torch.equal(other[2], first[2]) and A.bar_ratio(other[2], first[2].cpu()) > 100.0
    seed.fill_(SEED)
    assert same(first, training_step(tag, L, plan, params, packed, ws=ws))


# ---- 4. nothing else moves ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["narrow", "ch24"])
def test_everything_but_the_training_step_ignores_the_setting(tag):
    """A plan with p = 0.25 set against a plan that never heard of dropout: training = 0 calls and the Heun sampler are bit-identical;
    after set_dropout(0, None) so is the whole training step."""
    from tests.test_hip_adm_arch import infer
    cfg, B, H, W = A.ARCHS[tag]
    L, plain, params, packed = build(tag)
    _, plan, _, packed2 = build(tag)
    plan.set_dropout(P, seed_tensor(SEED))
    for kind in [k for _, k in A.runs(tag)]:
        for a, b in zip(infer(tag, plain, packed, kind), infer(tag, plan, packed2, kind)):
            assert (a is None and b is None) or torch.equal(a, b), (tag, kind)
    if tag not in A.PLAIN:
        cond, m, init, _ = fx.sampler_inputs("det_u", B, H, W)
        sd = L.sampler_desc(orc.SamplerParams(timesteps=3))
        xs = [pl.sample(pk, sd, dev(cond), dev(m), dev(init), None, return_last=True) for pl, pk in ((plain, packed), (plan, packed2))]
        assert torch.equal(xs[0], xs[1]) and bool(torch.isfinite(xs[0]).all())
    want = training_step(tag, L, plain, params, packed)
    assert not same(want, training_step(tag, L, plan, params, packed2))
    plan.set_dropout(0.0, None)
    assert same(want, training_step(tag, L, plan, params, packed2))


@pytest.mark.parametrize("tag", D.ROWS)
def test_p0_launches_what_the_parent_launched(tag):
    L, plan, params, packed = net(tag)
    training_step(tag, L, plan, params, packed)
    _, rows = profiled(L, lambda: training_step(tag, L, plan, params, packed))
    print(f"{tag}: {sum(rows.values())} launches in {len(rows)} rows (the parent: {sum(PARENT_ROWS[tag].values())} in {len(PARENT_ROWS[tag])})")
    assert dict(rows) == PARENT_ROWS[tag], (sorted(set(rows.items()) ^ set(PARENT_ROWS[tag].items())))
