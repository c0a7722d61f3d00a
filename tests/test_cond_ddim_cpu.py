"""CPU checks of PlCondDdim on the ADM U-Net (reference models/ddim.py:1053-1605, configs/model/adm_cond_h_res32.yaml): the
self-conditioning network's parameter table, the module's state_dict against the reference's (tests/golden/cond_ddim.npz), the
configurations that are not built, and the new C entry points in the header and the binding."""
import os
import re

import numpy as np
import pytest

import mcedm_amd  # noqa: F401
from mcedm_amd import lib as L
from oracle import mcedm_oracle as orc
from tests.test_hip_module import hparams, wrap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "cond_ddim.npz")
NEW = ["mcedm_eps_noise_inputs", "mcedm_eps_self_cond", "mcedm_eps_loss", "mcedm_unet_backward", "mcedm_unet_backward_bucketed",
       "mcedm_vp_sampler_workspace_bytes", "mcedm_vp_heun_sample", "mcedm_vp_heun_sample_rng"]


def ddim_hparams(name="adm_cond_h", **model):
    hp = hparams(orc.UNetConfig(in_channels=1, cond_channels=1, out_ch=1), timesteps=50, S_churn=15.0)
    hp["name"] = name
    hp.model.update(type="simple", var_type="fixedsmall", node_type=False, self_cond=True, cond_p=1.0)
    hp.model.update(model)
    hp["diffusion"] = wrap(dict(beta_schedule="linear", beta_start=0.0001, beta_end=0.02, num_diffusion_timesteps=1000))
    return hp


def test_self_cond_plan_parameter_table_is_the_references():
    """adm_blocks.py:227-238: conv_in reads cat(cond, x_self_cond, x) -> the cat_cond table with cond + in conditioning channels."""
    from mcedm_amd.adm_blocks import DhariwalUNet
    net = DhariwalUNet(ddim_hparams())
    assert net.self_condition and net.in_channels == 3 and net.cond_channels == 1 and net.plan_cond_channels == 2
    ref = orc.param_shapes(orc.UNetConfig(in_channels=1, cond_channels=2, out_ch=1))
    assert [(n, tuple(p.shape)) for n, p in net.named_parameters()] == [(n, tuple(s)) for n, s in ref]
    plan = net.plan                       # the HIP plan's own table agrees with the module's (checked on creation)
    assert plan.param_shapes[4] == (64, 3, 3, 3) and plan.cond_channels == 2


def test_state_dict_keys_match_the_reference():
    from mcedm_amd.ddim import PlCondDdim
    m = PlCondDdim(ddim_hparams())
    keys = [str(k) for k in np.load(GOLDEN)["state_dict_keys"]]
    assert list(m.state_dict().keys()) == keys
    assert m.cond_p == 1.0 and m.num_timesteps == 1000 and m.model.self_condition
    assert PlCondDdim(ddim_hparams(cond_p=0.8)).cond_p == 0.8


def test_unbuilt_configurations_raise():
    from mcedm_amd.ddim import PlCondDdim, PlCondEdm
    from mcedm_amd.mcedm import PlMcedm
    with pytest.raises(NotImplementedError, match="DDPM U-Net"):
        PlCondDdim(ddim_hparams(name="ddim_cond_h"))
    with pytest.raises(NotImplementedError, match="dx_cond"):
        PlCondDdim(ddim_hparams(dx_cond=True))
    hp = ddim_hparams()
    hp.optimization.pde_loss_lambda = 0.1
    with pytest.raises(NotImplementedError, match="pde_loss_lambda"):
        PlCondDdim(hp)
    m = PlCondDdim(ddim_hparams())
    with pytest.raises(NotImplementedError, match="1452-1531"):
        m.sample(None, None, None)
    with pytest.raises(NotImplementedError, match="guide_dx"):
        m.sample_edm(None, None, m.sparams, guide_dx=True)
    with pytest.raises(NotImplementedError, match="self_cond"):          # PlCondEdm's sampler feeds `denoised` back: not built
        PlCondEdm(ddim_hparams(name="adm_edm_cond_h"))
    hp = hparams(orc.UNetConfig())
    hp.model.self_cond = True
    with pytest.raises(NotImplementedError, match="self_cond"):
        PlMcedm(hp)


def test_new_entries_declared_in_header_and_binding():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mcedm_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(mcedm_[a-z0-9_]+)\s*\(", src))
    lib = L.load()
    for n in NEW:
        assert n in declared and n in L.EXPORTS, n
        getattr(lib, n)
    assert lib.mcedm_version() == L.ABI_VERSION == 4


def test_vp_sampler_workspace_is_the_forward_plus_state():
    plan = L.Plan(1, 2, 1, 64, (1, 1, 1), 1, (32,), 128)
    B, H, W = 3, 32, 32
    state = 3 * B * H * W * 8 + 2 * B * H * W * 4 + B * 2 * H * W * 4
    assert plan.vp_sampler_workspace_bytes(B, H, W) >= plan.workspace_bytes(B, H, W) + state
