"""CPU checks of PlCondDdim on the DDPM U-Net ``Model`` (reference models/ddim.py:43-46, configs/model/ddim_cond_h_res32.yaml) and of
the cond_enc / combine_enc head of its plan: the parameter table and the module's state_dict against the reference's
(tests/golden/ddpm_cond.npz), what still raises, the new C entries in header, binding and library, and their host-side
rejections (which run before any launch, so without a GPU), with those of the unconditional entries and of the size queries."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import mcedm_amd  # noqa: F401
from mcedm_amd import lib as L
from tests import _ddpm_cond as D
from tests.test_hip_module import wrap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ddpm_cond.npz")
NEW = ["mcedm_ddpm_plan_create_cond", "mcedm_ddpm_cond_map", "mcedm_ddpm_forward_cond", "mcedm_ddpm_vp_sampler_workspace_bytes",
       "mcedm_ddpm_vp_heun_sample", "mcedm_ddpm_vp_heun_sample_rng", "mcedm_ddpm_cond_ddim_workspace_bytes",
       "mcedm_ddpm_cond_ddim_sample", "mcedm_ddpm_cond_ddim_sample_rng"]


def cond_plan(cond_channels=1, **over):
    c = D.CFG
    kw = dict(in_channels=c.in_channels, out_channels=c.out_ch, ch=c.ch, ch_mult=c.ch_mult, num_res_blocks=c.num_res_blocks,
              attn_resolutions=c.attn_resolutions, resolution=c.resolution, self_cond=True, cond_channels=cond_channels)
    kw.update(over)
    return L.DdpmPlan(**kw)


def module(**kw):
    from mcedm_amd.ddim import PlCondDdim
    return PlCondDdim(wrap(D.hparams_dict(**kw)))


@pytest.mark.parametrize("cc,key", [(1, "state_dict_keys"), (2, "state_dict_keys_node")])
def test_plan_parameter_table_is_the_references(cc, key):
    """Names in Model.state_dict() order (cond_enc.* / combine_enc.* behind conv_in.*), shapes of the reference's modules."""
    keys = [str(k) for k in np.load(GOLDEN)[key]]
    names = [k[len("model."):] for k in keys if k.startswith("model.")]
    plan = cond_plan(cc)
    assert plan.param_names == names
    assert plan.param_shapes == [tuple(s) for _, s in D.param_shapes(cc)]
    at = names.index("conv_in.bias") + 1
    assert names[at:at + 6] == [n for n, _ in D.head_shapes(cc)] and plan.param_shapes[at - 2] == (64, 2, 3, 3)
    plain = cond_plan(0)                    # a plan without the head: the old table, a smaller packed buffer
    assert plain.param_names == [n for n in names if not n.startswith(("cond_enc", "combine_enc"))]
    assert plain.packed_bytes < plan.packed_bytes and plain.workspace_bytes(3) == plan.workspace_bytes(3)


@pytest.mark.parametrize("node_type,key", [(False, "state_dict_keys"), (True, "state_dict_keys_node")])
def test_module_constructs_with_the_shipped_hparams(node_type, key):
    m = module(node_type=node_type)
    assert list(m.state_dict().keys()) == [str(k) for k in np.load(GOLDEN)[key]]
    net = m.model
    assert type(net).__name__ == "Model" and net.self_condition and not net.cat_condition
    assert net.cond_channels == (2 if node_type else 1) and net.plan.cond_channels == net.cond_channels
    assert net.cond_enc[2].padding_mode == "circular" and isinstance(net.cond_enc[1], torch.nn.GELU)
    assert m.cond_p == 1.0 and m.num_timesteps == 1000
    assert "optimizer" in m.configure_optimizers()


def test_training_raises_and_cat_cond_stays_unbuilt():
    m = module()
    with pytest.raises(NotImplementedError, match="no backward"):
        m.training_step((None, None, None, None), 0)
    with pytest.raises(NotImplementedError, match="no backward"):
        m.forward(None, None, None)
    hp = wrap(D.hparams_dict())
    hp.model.cat_cond = True
    from mcedm_amd.ddim import PlCondDdim
    with pytest.raises(NotImplementedError, match="DDPM U-Net"):
        PlCondDdim(hp)
    for flag, val, msg in (("dx_cond", True, "dx_cond"), ("dropout", 0.1, "dropout"), ("resamp_with_conv", False, "resamp_with_conv"),
                           ("type", "bayesian", "bayesian")):
        hp = wrap(D.hparams_dict())
        hp.model[flag] = val
        with pytest.raises(NotImplementedError, match=msg):
            PlCondDdim(hp)
    with pytest.raises(NotImplementedError, match="guide_dx"):
        m.sample_edm(None, None, m.sparams, guide_dx=True)


def test_new_entries_in_header_binding_and_library():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mcedm_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(mcedm_[a-z0-9_]+)\s*\(", src))
    nm = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (mcedm_[a-z0-9_]+)$", nm, flags=re.M))
    lib = L.load()
    for n in NEW:
        assert n in declared and n in L.EXPORTS and n in exported, n
        getattr(lib, n)
    assert "mcedm_ddpm_cond_desc" in src and lib.mcedm_version() == L.ABI_VERSION == 4


def _last():
    return L.load().mcedm_last_error().decode()


def test_host_side_rejections():
    """cat_cond != 0; NULL cond on a plan with cond_channels > 0; a short workspace; a map / a conditioned sampler on a plan
    without the head.  The pointers are never dereferenced: every check runs on the host before the first launch."""
    lib = L.load()
    with pytest.raises(RuntimeError, match=r"\(-1\).*cat_cond"):
        cond_plan(1, cat_cond=True)
    with pytest.raises(RuntimeError, match=r"\(-1\).*cond_channels"):
        cond_plan(65)
    plan, plain = cond_plan(1), cond_plan(0)
    one = C.c_void_p(4096)
    B = 3
    assert lib.mcedm_ddpm_cond_map(plan._h, one, None, one, B, None) == -1 and "cond is null" in _last()
    assert lib.mcedm_ddpm_cond_map(plain._h, one, one, one, B, None) == -1 and "without the cond_enc head" in _last()
    need = plan.workspace_bytes(B)
    assert lib.mcedm_ddpm_forward_cond(plan._h, one, one, None, one, 500.0, one, one, need - 1, B, None) == -3
    assert "workspace too small" in _last()
    assert lib.mcedm_ddpm_forward_cond(plain._h, one, one, None, one, 500.0, one, one, need, B, None) == -1
    assert "without the cond_enc head" in _last()
    # the two samplers
    vd = L.vp_sampler_desc(2, 1, [5.0, 1.0, 0.0], [5.0, 1.0], [900.0, 800.0, 700.0, 0.0], 1.0, 0.0)
    need = plan.vp_sampler_workspace_bytes(B)
    assert need >= plan.workspace_bytes(B) + 3 * B * 1024 * 8 + 3 * B * 1024 * 4 + B * 64 * 1024 * 4
    vp = lambda p, d, cond, nbytes: lib.mcedm_ddpm_vp_heun_sample(p._h, one, C.byref(d), cond, one, None, one, 1, one, nbytes, B, None)   # noqa: E731
    assert vp(plan, vd, None, need) == -1 and "cond goes with cond_channels" in _last()
    assert vp(plan, vd, one, need - 1) == -3 and "workspace too small" in _last()
    assert vp(plain, vd, one, need) == -1 and "neither 0 nor the plan's 0" in _last()
    churn = L.vp_sampler_desc(2, 1, [5.0, 1.0, 0.0], [6.0, 1.0], [900.0, 800.0, 700.0, 0.0], 1.0, 0.0)
    assert vp(plan, churn, one, need) == -1 and "needs step_noise" in _last()
    assert lib.mcedm_ddpm_vp_heun_sample_rng(plan._h, one, C.byref(vd), one, one, None, one, 1, one, need, B, None) == -1
    assert "rng_seed" in _last()
    ae = torch.cumprod(1 - torch.cat([torch.zeros(1), torch.linspace(1e-4, 0.02, 1000)]), 0)
    sp = wrap(D.ddim_sampler(4, w=0.5))
    dd = L.cond_ddim_desc(sp, ae, 1, True)
    need = plan.cond_ddim_workspace_bytes(B)
    dm = lambda p, d, cond, nbytes: lib.mcedm_ddpm_cond_ddim_sample(p._h, one, C.byref(d), cond, one, None, one, one, 1, one, nbytes, B, None)   # noqa: E731
    assert dm(plan, dd, None, need) == -1 and "cond goes with cond_channels" in _last()
    assert dm(plan, dd, one, need - 1) == -3 and "workspace too small" in _last()
    assert dm(plan, L.cond_ddim_desc(wrap(D.ddim_sampler(4, eta=0.5)), ae, 1, True), one, need) == -1 and "eta != 0 needs eta_noise" in _last()
    noself = cond_plan(1, self_cond=False)
    assert dm(noself, dd, one, need) == -1 and "built without it" in _last()
    assert lib.mcedm_ddpm_cond_ddim_sample_rng(plan._h, one, C.byref(dd), one, one, None, one, one, 1, one, need, B, None) == -1
    assert "rng_seed" in _last()


def _samplers():
    """Of the two unconditional samplers: the makers of their descriptions (each returns (desc, keepalive)) and
    call(plan, packed, workspace, nbytes, B, made)."""
    from oracle import ddpm_oracle as ddo
    lib, one = L.load(), C.c_void_p(4096)
    betas = ddo.betas_of(D.CFG)
    ae = ddo.alphas_ext_of(betas)

    def rp(**kw):
        return L.repaint_desc(ddo.RepaintParams(timesteps=3, n_time_u=8, **kw), ddo.edm_steps_of(betas), ae, 1, 0)

    def dd(self_cond):
        return L.ddim_desc(ddo.DdimParams(timesteps=3, n_repeat=1, n_time_h=8), ae, 1, 0, self_cond)

    def repaint(p, pk, ws, nbytes, b, made):
        return lib.mcedm_repaint_sample(p, pk, C.byref(made[0]), one, one, None, one, one, 1, ws, nbytes, b, None)

    def ddim(p, pk, ws, nbytes, b, made):
        return lib.mcedm_ddim_repaint_sample(p, pk, C.byref(made[0]), one, one, None, one, one, 1, ws, nbytes, b, None)
    return rp, dd, repaint, ddim


def test_host_side_rejections_of_the_unconditional_entries():
    """mcedm_ddpm_forward, _forward_sc, _denoise, mcedm_repaint_sample, mcedm_ddim_repaint_sample and the six size queries: a null
    plan / packed / workspace, an empty batch, a workspace one byte short (the text names the bytes needed), x_self_cond on a plan
    without self-conditioning, and which check speaks when two fail at once.  All on the host, before any launch."""
    lib = L.load()
    plan, noself = cond_plan(0), cond_plan(0, self_cond=False)
    one = C.c_void_p(4096)
    B = 3
    rp, dd, repaint, ddim = _samplers()
    rd, dsc, net = rp(), dd(True), plan.workspace_bytes(B)
    entries = {
        "ddpm_forward": (net, lambda p, pk, ws, n, b: lib.mcedm_ddpm_forward(p, pk, one, 500.0, one, ws, n, b, None)),
        "ddpm_forward_sc": (net, lambda p, pk, ws, n, b: lib.mcedm_ddpm_forward_sc(p, pk, one, one, 500.0, one, ws, n, b, None)),
        "ddpm_denoise": (net, lambda p, pk, ws, n, b: lib.mcedm_ddpm_denoise(p, pk, one, 1.5, 700.0, one, None, ws, n, b, None)),
        "repaint_sample": (plan.repaint_workspace_bytes(B), lambda p, pk, ws, n, b: repaint(p, pk, ws, n, b, rd)),
        "ddim_repaint_sample": (plan.ddim_workspace_bytes(B), lambda p, pk, ws, n, b: ddim(p, pk, ws, n, b, dsc)),
    }
    for who, (need, call) in entries.items():
        for args in ((None, one, one), (plan._h, None, one), (plan._h, one, None)):
            assert call(*args, need, B) == -1 and _last() == f"{who}: null argument", (who, args)
        assert call(plan._h, one, one, need, 0) == -1 and _last() == "ddpm: empty batch", who
        assert call(plan._h, one, one, need - 1, B) == -3, who
        assert _last() == f"{who}: workspace too small ({need - 1} < {need} bytes)", who
        # two at once: the empty batch speaks before the workspace
        assert call(plan._h, one, one, 0, 0) == -1 and _last() == "ddpm: empty batch", who
    # x_self_cond given to a plan built without self-conditioning (it speaks before the empty batch and the workspace)
    need = noself.workspace_bytes(B)
    assert lib.mcedm_ddpm_forward_sc(noself._h, one, one, one, 500.0, one, one, need, B, None) == -1
    assert _last() == "ddpm_forward_sc: the network was built without self-conditioning channels"
    assert lib.mcedm_ddpm_forward_sc(noself._h, one, one, one, 500.0, one, one, 0, 0, None) == -1 and "without self-conditioning" in _last()
    assert lib.mcedm_ddpm_forward_sc(noself._h, one, one, None, 500.0, one, one, need - 1, B, None) == -3     # None: as mcedm_ddpm_forward
    assert ddim(noself._h, one, one, noself.ddim_workspace_bytes(B), B, dsc) == -1
    assert _last() == "ddim_repaint_sample: self-conditioning asked of a network built without it"
    assert ddim(noself._h, one, one, noself.ddim_workspace_bytes(B) - 1, B, dd(False)) == -3
    # two at once on the samplers: the schedule speaks before the workspace
    assert repaint(plan._h, one, one, 0, B, rp(w=0.5)) == -1 and "classifier-free guidance needs a conditional network" in _last()
    bad = rp()
    bad[0].timesteps = 1
    assert repaint(plan._h, one, one, 0, B, bad) == -1 and "timesteps=1 n_repeat=2 out of range" in _last()
    bad = dd(True)
    bad[0].skip_type = 2
    assert ddim(plan._h, one, one, 0, B, bad) == -1 and "skip_type must be 0 (uniform) or 1 (quad)" in _last()
    # the size queries
    cat = cond_plan(1, self_cond=False, cat_cond=True)
    sz = C.c_size_t()
    for q in ("ddpm_workspace_bytes", "repaint_workspace_bytes", "ddim_workspace_bytes", "ddpm_vp_sampler_workspace_bytes",
              "ddpm_cond_ddim_workspace_bytes", "ddpm_edm_sampler_workspace_bytes"):
        fn = getattr(lib, "mcedm_" + q)
        for pl in (plan, cat):
            assert fn(None, B, C.byref(sz)) == -1 and _last() == f"{q}: null argument", q
            assert fn(pl._h, B, None) == -1 and _last() == f"{q}: null argument", q
            assert fn(pl._h, 0, C.byref(sz)) == -1 and _last() == "ddpm: empty batch", q
            assert fn(pl._h, -2, C.byref(sz)) == -1 and _last() == "ddpm: empty batch", q
