"""CPU checks of PlCondEdm on the DDPM U-Net ``Model`` with the conditioning concatenated to its input (reference
models/ddim.py:1608-1773, configs/model/edm_cond_h_res32.yaml): the plan's and the module's parameter tables against the
reference's state_dict (tests/golden/ddpm_edm.npz), what raises, the new C entries in header, binding and library, and their
host-side rejections (which run before any launch, so without a GPU)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import mcedm_amd  # noqa: F401
from mcedm_amd import lib as L
from tests import _ddpm_edm as D
from tests.test_hip_module import wrap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ddpm_edm.npz")
NEW = ["mcedm_ddpm_forward_cat", "mcedm_ddpm_edm_denoise", "mcedm_ddpm_edm_sampler_workspace_bytes", "mcedm_ddpm_edm_heun_sample",
       "mcedm_ddpm_edm_heun_sample_rng"]


def cat_plan(cond_channels=1, cat_cond=True, **over):
    c = D.CFG
    kw = dict(in_channels=c.in_channels, out_channels=c.out_ch, ch=c.ch, ch_mult=c.ch_mult, num_res_blocks=c.num_res_blocks,
              attn_resolutions=c.attn_resolutions, resolution=c.resolution, self_cond=False, cond_channels=cond_channels,
              cat_cond=cat_cond)
    kw.update(over)
    return L.DdpmPlan(**kw)


def module(**kw):
    from mcedm_amd.ddim import PlCondEdm
    return PlCondEdm(wrap(D.hparams_dict(**kw)))


@pytest.mark.parametrize("cc,key", [(1, "state_dict_keys"), (2, "state_dict_keys_node")])
def test_plan_parameter_table_is_the_references(cc, key):
    """Model.state_dict() order without cond_enc.* / combine_enc.*; conv_in reads cond_channels + in_channels planes."""
    keys = [str(k) for k in np.load(GOLDEN)[key]]
    names = [k[len("model."):] for k in keys if k.startswith("model.")]
    assert not [n for n in names if n.startswith(("cond_enc", "combine_enc"))]
    plan = cat_plan(cc)
    assert plan.param_names == names and plan.cat_cond and plan.cond_channels == cc
    assert plan.param_shapes == [tuple(s) for _, s in D.param_shapes(cc)]
    assert plan.param_shapes[names.index("conv_in.weight")] == (64, cc + 1, 3, 3)
    plain = cat_plan(0, cat_cond=False)      # the plan without conditioning: same names, a narrower conv_in, no guidance buffer
    assert plain.param_names == names and plain.param_shapes[names.index("conv_in.weight")] == (64, 1, 3, 3)
    assert plain.workspace_bytes(3) < plan.workspace_bytes(3) <= plain.workspace_bytes(3) + 3 * 1024 * 4 + 512


@pytest.mark.parametrize("node_type,key", [(False, "state_dict_keys"), (True, "state_dict_keys_node")])
def test_module_constructs_with_the_shipped_hparams(node_type, key):
    m = module(node_type=node_type)
    assert list(m.state_dict().keys()) == [str(k) for k in np.load(GOLDEN)[key]]
    net = m.model
    cc = 2 if node_type else 1
    assert type(net).__name__ == "Model" and net.cat_condition and not net.self_condition
    assert net.cond_enc is None and net.combine_enc is None and tuple(net.conv_in.weight.shape) == (64, cc + 1, 3, 3)
    assert net.cond_channels == cc and net.plan.cond_channels == cc and net.plan.cat_cond
    assert type(m.ema_model.ma_model).__name__ == "Model"
    assert (m.sigma_data, m.sigma_min, m.sigma_max, m.cond_p, m.num_timesteps) == (1.0, 0.002, 80, 1.0, 1000)
    assert "optimizer" in m.configure_optimizers()


def test_sampler_configuration_behaves_as_on_the_adm_network():
    m = module()
    sp = m.get_edm_sampler_params()
    assert (sp.type, sp.timesteps, sp.S_churn, sp.n_samples, sp.w) == ("edm", 50, 15.0, 5, 0.0)
    m.set_test_sampler_params(wrap(dict(D.sampler_dict(), type="ddim")))      # not an EDM sampler: the default EDM one instead
    assert m.test_sparams.type == "edm" and m.test_sparams.timesteps == 50
    mine = wrap(D.sampler_dict())
    m.set_test_sampler_params(mine)
    assert m.test_sparams is mine
    s = torch.tensor([0.3, 7.0], dtype=torch.float64)
    assert m.round_sigma(s) is s and m.round_sigma(s, return_index=True) == 0 and float(m.round_sigma(2.5)) == 2.5


def test_what_raises():
    from mcedm_amd.ddim import PlCondDdim, PlCondEdm
    from mcedm_amd.ddim_blocks import Model
    m = module()
    with pytest.raises(NotImplementedError, match="no backward"):
        m.training_step((None, None, None, None), 0)
    with pytest.raises(NotImplementedError, match="no backward"):
        m.forward(None, None, None)
    with pytest.raises(NotImplementedError, match="dx_cond"):
        PlCondEdm(wrap(D.hparams_dict(dx_cond=True, dx_norm="prob")))
    with pytest.raises(NotImplementedError, match="self_cond"):
        PlCondEdm(wrap(D.hparams_dict(self_cond=True)))
    with pytest.raises(NotImplementedError, match="one noise level for the whole batch"):
        m.model_precond(torch.zeros(3, 1, 32, 32), torch.tensor([1.0, 1.0, 2.0]))
    with pytest.raises(NotImplementedError, match="x_self_cond"):
        m.get_denoised(m.model, torch.zeros(3, 1, 32, 32), torch.tensor(1.0), x_self_cond=torch.zeros(3, 1, 32, 32))
    with pytest.raises(NotImplementedError, match="dx_cond"):
        m.get_denoised(m.model, torch.zeros(3, 1, 32, 32), torch.tensor(1.0), dx=torch.zeros(3, 1, 32, 32))
    with pytest.raises(NotImplementedError, match="Only EDM sampler"):
        m.sample(None, None, None)
    # Model: cat_cond together with self_cond keeps its text; PlCondDdim refuses cat_cond on this network whatever self_cond is
    hp = wrap(D.hparams_dict(self_cond=True))
    with pytest.raises(NotImplementedError, match="cat_cond on the DDPM U-Net"):
        Model(hp)
    for sc in (False, True):
        hp = wrap(D.hparams_dict(self_cond=sc))
        hp["name"] = "ddim_cond_h"
        with pytest.raises(NotImplementedError, match="DDPM U-Net"):
            PlCondDdim(hp)
    assert Model(wrap(D.hparams_dict())).cat_condition


def test_new_entries_in_header_binding_and_library():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mcedm_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(mcedm_[a-z0-9_]+)\s*\(", src))
    nm = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (mcedm_[a-z0-9_]+)$", nm, flags=re.M))
    lib = L.load()
    for n in NEW:
        assert n in declared and n in L.EXPORTS and n in exported, n
        getattr(lib, n)
    assert L.SAMPLER_STEMS["mcedm_ddpm_edm_heun_sample"] == 1 and issubclass(L.GraphedDdpmEdmSampler, L._GraphedCall)
    assert lib.mcedm_version() == L.ABI_VERSION == 4


def _last():
    return L.load().mcedm_last_error().decode()


def test_host_side_rejections():
    """Null arguments, a short workspace, cond on a plan without cond channels, cat_cond with self_cond, guidance without cond, a
    churning schedule without draws.  The pointers are never dereferenced: every check runs on the host before the first launch."""
    lib = L.load()
    with pytest.raises(RuntimeError, match=r"\(-1\).*cat_cond"):
        cat_plan(1, self_cond=True)
    with pytest.raises(RuntimeError, match=r"\(-1\).*at most 64"):
        cat_plan(64)
    plan, plain = cat_plan(1), cat_plan(0, cat_cond=False)
    one = C.c_void_p(4096)
    B = 3
    need = plan.workspace_bytes(B)
    fc = lambda p, x, cond, nbytes: lib.mcedm_ddpm_forward_cat(p._h, one, x, cond, -0.75, one, one, nbytes, B, None)   # noqa: E731
    assert fc(plan, None, one, need) == -1 and "null argument" in _last()
    assert fc(plan, one, one, need - 1) == -3 and "workspace too small" in _last()
    assert fc(plain, one, one, need) == -1 and "without cat_cond channels" in _last()
    dn = lambda p, x, cond, sigma, nbytes: lib.mcedm_ddpm_edm_denoise(p._h, one, x, cond, sigma, 0.1, 0.5, 1.0, one, None, one, nbytes, B, None)   # noqa: E731
    assert dn(plan, None, one, 1.5, need) == -1 and "null argument" in _last()
    assert dn(plan, one, one, 0.0, need) == -1 and "must be positive" in _last()
    assert dn(plan, one, one, 1.5, need - 1) == -3 and "workspace too small" in _last()
    assert dn(plain, one, one, 1.5, need) == -1 and "without cat_cond channels" in _last()
    # the sampler
    vd = L.vp_sampler_desc(2, 1, [5.0, 1.0, 0.0], [5.0, 1.0], [0.4, 0.0, 0.0, 0.0], 1.0, 0.0)
    vd0 = L.vp_sampler_desc(2, 0, [5.0, 1.0, 0.0], [5.0, 1.0], [0.4, 0.0, 0.0, 0.0], 1.0, 0.0)
    need = plan.edm_sampler_workspace_bytes(B)
    assert need >= plan.workspace_bytes(B) + 3 * B * 1024 * 8 + 4 * B * 1024 * 4
    gd = L.GuidanceDesc(1, 0.01, 0.1, 0.2, 1.4, 0.05, 0.0, 0.1, 5.0)
    sm = lambda p, d, g, cond, nbytes, init=one: lib.mcedm_ddpm_edm_heun_sample(   # noqa: E731
        p._h, one, C.byref(d), 1.0, g, cond, init, None, one, 1, one, nbytes, B, None)
    assert sm(plan, vd, None, one, need, init=None) == -1 and "null argument" in _last()
    assert sm(plan, vd, None, one, need - 1) == -3 and "workspace too small" in _last()
    assert sm(plain, vd, None, one, need) == -1 and "without cat_cond channels" in _last()
    assert sm(plan, vd, None, None, need) == -1 and "cond_channels 1, expected 0" in _last()
    assert sm(plan, vd0, None, one, need) == -1 and "cond_channels 0, expected 1" in _last()
    assert sm(plan, vd0, C.byref(gd), None, need) == -1 and "PDE guidance" in _last()
    bad = L.GuidanceDesc(3, 0.01, 0.1, 0.2, 1.4, 0.05, 0.0, 0.1, 5.0)
    assert sm(plan, vd, C.byref(bad), one, need) == -1 and "guidance system" in _last()
    churn = L.vp_sampler_desc(2, 1, [5.0, 1.0, 0.0], [6.0, 1.0], [0.4, 0.0, 0.0, 0.0], 1.0, 0.0)
    assert sm(plan, churn, None, one, need) == -1 and "needs step_noise" in _last()
    assert lib.mcedm_ddpm_edm_heun_sample_rng(plan._h, one, C.byref(vd), 1.0, None, one, one, None, one, 1, one, need, B, None) == -1
    assert "rng_seed" in _last()
    assert lib.mcedm_ddpm_edm_heun_sample(plan._h, one, C.byref(vd), 0.0, None, one, one, None, one, 1, one, need, B, None) == -1
    assert "sigma_data" in _last()
