"""CPU: dropout of the ADM U-Net before any kernel is involved.

1. The oracle with injected masks (tests/_adm_dropout.py) reproduces what the REFERENCE's DhariwalUNet computed in train() mode with
   dropout = 0.25 and the same masks (tests/golden/adm_dropout.npz, tools/make_golden_adm_dropout.py), at the project's bar: position
   of the dropout, its scale and the train / eval semantics are pinned against the reference.
2. hparams.model.dropout: what the four drop-in constructors accept and refuse.
3. mcedm_unet_plan_set_dropout: the arguments it refuses, and the workspace sizes it does and does not change.
"""
import ctypes as C
import math

import pytest
import torch

import mcedm_amd  # noqa: F401
from mcedm_amd import lib as L
from oracle import fixtures as fx
from tests import _adm_arch as A
from tests import _adm_dropout as D
from tests.test_cond_ddim_cpu import ddim_hparams
from tests.test_ddpm_cond_cpu import module as ddpm_module
from tests.test_hip_cond_edm import cond_hparams
from tests.test_hip_module import hparams


# ---- 1. the oracle with injected masks against the reference's run -----------------------------------------------------------------------
@pytest.mark.parametrize("tag", D.GOLDEN_ROWS)
def test_injected_oracle_reproduces_the_reference(golden, tag):
    g = golden("adm_dropout.npz")
    assert int(g["seed"]) == D.SEED and float(g["p"]) == D.P_DROP
    cfg, B, H, W = A.ARCHS[tag]
    masks = D.masks_for(cfg, B, H, W, D.P_DROP, D.SEED)
    kept = sum(float(m.sum()) for m in masks.values()) / sum(m.numel() for m in masks.values())
    assert abs(kept - (1 - D.P_DROP)) < 0.01, kept
    loss, grads = D.training_grads(tag, masks)
    F = D.forward_F(tag, masks)
    r_f = A.bar_ratio(torch.as_tensor(g[f"{tag}::F"]), F)
    r_l = A.bar_ratio(torch.as_tensor(g[f"{tag}::loss"]).reshape(1), loss.reshape(1))
    norms = torch.tensor([math.sqrt(float((v ** 2).sum())) for v in grads.values()], dtype=torch.float64)
    r_n = A.bar_ratio(torch.as_tensor(g[f"{tag}::grad_sqnorm_each"]).sqrt(), norms)
    r_g, n_g = max((A.bar_ratio(torch.as_tensor(g[f"{tag}::grad::{n}"]), grads[n]), n) for n in D.golden_grad_names(tag))
    print(f"{tag}: reference fp32 run vs the fp64 oracle with injected masks, worst err / bar: F {r_f:.4f}, loss {r_l:.4f}, "
          f"gradient norms {r_n:.4f}, stored gradients {r_g:.4f} ({n_g})")
    assert max(r_f, r_l, r_n, r_g) <= 1.0
    # eval(): the reference in eval() mode is the dropout = 0 network, i.e. the oracle as it stands
    with torch.no_grad():
        F0 = D.training_F(tag, A.params(tag, torch.float64))
    assert A.bar_ratio(torch.as_tensor(g[f"{tag}::F_eval"]), F0) <= 1.0
    assert A.bar_ratio(torch.as_tensor(g[f"{tag}::F"]), F0) > 100.0                 # and dropout matters


def test_another_seed_and_another_block_give_other_masks():
    cfg, B, H, W = A.ARCHS["narrow"]
    a = D.masks_for(cfg, B, H, W, D.P_DROP, D.SEED)
    b = D.masks_for(cfg, B, H, W, D.P_DROP, D.SEED + 1)
    keys = list(a)
    assert all(not torch.equal(a[k], b[k]) for k in keys)
    same_shape = [(k1, k2) for i, k1 in enumerate(keys) for k2 in keys[i + 1:] if a[k1].shape == a[k2].shape]
    assert same_shape and all(not torch.equal(a[k1], a[k2]) for k1, k2 in same_shape)


# ---- 2. hparams -------------------------------------------------------------------------------------------------------------------------
def _adm_hparams(kind, dropout):
    hp = {"unet": hparams(fx.CFG_P), "mcedm": hparams(fx.CFG_P), "cond_edm": cond_hparams(), "cond_ddim": ddim_hparams()}[kind]
    hp.model.dropout = dropout
    return hp


def _construct(kind, dropout):
    from mcedm_amd.adm_blocks import DhariwalUNet
    from mcedm_amd.ddim import PlCondDdim, PlCondEdm
    from mcedm_amd.mcedm import PlMcedm
    cls = {"unet": DhariwalUNet, "mcedm": PlMcedm, "cond_edm": PlCondEdm, "cond_ddim": PlCondDdim}[kind]
    return cls(_adm_hparams(kind, dropout))


@pytest.mark.parametrize("kind", ["unet", "mcedm", "cond_edm", "cond_ddim"])
def test_dropout_constructs(kind):
    m = _construct(kind, 0.1)
    net = m if kind == "unet" else m.model
    assert net.dropout == 0.1 and type(net).__name__ == "DhariwalUNet"
    if kind != "unet" and m.ema_model is not None:
        assert m.ema_model.ma_model.dropout == 0.1          # the copy carries the knob; no training loss ever runs on it
    assert _construct(kind, 0.0).model.dropout == 0.0 if kind != "unet" else _construct(kind, 0.0).dropout == 0.0


@pytest.mark.parametrize("bad", [-0.1, 1.0, float("nan")])
@pytest.mark.parametrize("kind", ["unet", "mcedm", "cond_edm", "cond_ddim"])
def test_dropout_outside_the_unit_interval_is_a_value_error(kind, bad):
    with pytest.raises(ValueError, match="dropout"):
        _construct(kind, bad)


def test_the_ddpm_unet_still_refuses_dropout():
    from mcedm_amd.ddim import PlCondDdim
    from tests._ddpm_cond import hparams_dict
    from tests.test_hip_module import wrap
    hp = wrap(hparams_dict())
    hp.model["dropout"] = 0.1
    with pytest.raises(NotImplementedError, match="dropout"):
        PlCondDdim(hp)
    assert type(ddpm_module().model).__name__ == "Model"


# ---- 3. mcedm_unet_plan_set_dropout ---------------------------------------------------------------------------------------------------------
FAKE_SEED = 4096          # a non-NULL "device address": the setter and the size queries store it and never read through it


def _set(plan, p, seed):
    return L.load().mcedm_unet_plan_set_dropout(plan._h, C.c_double(p), seed)


def test_set_dropout_rejects_bad_arguments():
    plan = A.make_plan(L, A.cfg_of("narrow"))
    inval = L.abi.CONSTS["MCEDM_ERR_INVALID"]
    for p in (-0.1, 1.0, 1.5, float("nan"), float("inf"), 1.0 - 1e-12):       # the last one is 1.0f in fp32
        assert _set(plan, p, FAKE_SEED) == inval, p
        assert b"[0, 1)" in L.load().mcedm_last_error()
    assert _set(plan, 0.25, None) == inval and b"seed" in L.load().mcedm_last_error()
    assert L.load().mcedm_unet_plan_set_dropout(None, C.c_double(0.0), None) == inval
    assert _set(plan, 0.0, None) == 0 and _set(plan, 0.25, FAKE_SEED) == 0 and _set(plan, 0.0, FAKE_SEED) == 0
    for p in (-0.1, 1.0, float("nan")):
        with pytest.raises(ValueError):
            plan.set_dropout(p, None)
    with pytest.raises(ValueError):
        plan.set_dropout(0.25, None)
    assert "mcedm_unet_plan_set_dropout" in L.EXPORTS and {"mcedm_op_dropout_act", "mcedm_op_dropout_scale"} <= set(L.OP_EXPORTS)
    assert L.load().mcedm_version() == L.ABI_VERSION == 4


@pytest.mark.parametrize("tag", ["narrow", "ragged", "rect", "c128a", "ch24"])
def test_workspace_grows_by_the_saved_inputs_and_the_seed_slot(tag):
    cfg, B, H, W = A.ARCHS[tag]
    plan = A.make_plan(L, cfg)
    train0, infer0 = plan.workspace_bytes(B, H, W, True), plan.workspace_bytes(B, H, W, False)
    samp0 = plan.sampler_workspace_bytes(B, H, W) if cfg.in_channels == cfg.out_ch == 2 else None
    assert _set(plan, 0.25, FAKE_SEED) == 0
    align = lambda n: (n + 255) // 256 * 256      # noqa: E731
    extra = sum(align(4 * math.prod(shape)) for _, shape in D.block_shapes(cfg, B, H, W)) + align(8)
    assert plan.workspace_bytes(B, H, W, True) - train0 == extra
    assert plan.workspace_bytes(B, H, W, False) == infer0
    if samp0 is not None:
        assert plan.sampler_workspace_bytes(B, H, W) == samp0
    assert _set(plan, 0.0, None) == 0
    assert plan.workspace_bytes(B, H, W, True) == train0 and plan.workspace_bytes(B, H, W, False) == infer0
