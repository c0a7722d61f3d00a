"""CPU checks of dx_cond on PlCondDdim (reference models/ddim.py:199-204, 933-934, 1492, 1571, 1584): the new entries in header /
library / binding, the parameter table of the self_cond + dx network, what the constructor accepts and refuses, the host-side argument
checks of the new entries (they run before anything is enqueued), and the conditions the fixtures were recorded under."""
import ctypes as C
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest

import mcedm_amd  # noqa: F401
from mcedm_amd import lib as L
from oracle import mcedm_oracle as orc
from tests import _cond_dx as X
from tests import _cond_guided as G
from tests.test_cond_ddim_cpu import ddim_hparams
from tests.test_cond_ddim_sample_cpu import alphas_ext, sparams
from tests.test_cond_guided_cpu import gdesc, vp_desc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mcedm_vp_heun_sample_dxcond", "mcedm_vp_dxcond_workspace_bytes", "mcedm_cond_ddim_sample_dxcond",
       "mcedm_cond_ddim_dxcond_workspace_bytes", "mcedm_unet_backward_dx"]
Bq, R = 3, 32


def test_new_entries_in_header_library_and_binding():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mcedm_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(mcedm_[a-z0-9_]+)\s*\(", src))
    nm = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (mcedm_[a-z0-9_]+)$", nm, flags=re.M))
    lib = L.load()
    for n in NEW:
        assert n in declared and n in L.EXPORTS and n in exported, n
        assert getattr(lib, n).argtypes, n
    assert lib.mcedm_version() == L.ABI_VERSION == 4
    # a third table next to the two that the earlier suites pin; neither of those changed, and there is no _rng twin
    assert L.DXCOND_ENTRIES == {"mcedm_vp_heun_sample": "mcedm_vp_heun_sample_dxcond", "mcedm_cond_ddim_sample": "mcedm_cond_ddim_sample_dxcond"}
    assert not set(L.DXCOND_ENTRIES.values()) & (set(L.SAMPLER_STEMS) | set(L.GUIDED_ENTRIES.values()))
    assert {n[:-len("_rng")] for n in L.EXPORTS if n.endswith("_rng")} == set(L.SAMPLER_STEMS)
    assert len(L.GUIDED_ENTRIES) == 4 and "mcedm_heun_sample_dxcond" in L.SAMPLER_STEMS
    for stem, entry in L.DXCOND_ENTRIES.items():          # the guided signature plus one description
        assert len(getattr(lib, entry).argtypes) == len(getattr(lib, L.GUIDED_ENTRIES[stem]).argtypes) + 1, stem
    assert len(lib.mcedm_unet_backward_dx.argtypes) == len(lib.mcedm_unet_backward_bucketed.argtypes) + 1


@pytest.mark.parametrize("mode", X.MODES)
def test_self_cond_dx_parameter_table_is_the_references(mode):
    """adm_blocks.py:236-238, 266-280: conv_in reads cat(cond, x_self_cond, x[, dx]); dx_enc / combine_enc in front of enc."""
    from mcedm_amd.adm_blocks import DhariwalUNet
    net = DhariwalUNet(ddim_hparams(**X.model_update(mode)))
    assert net.self_condition and net.dx_cond and net.plan_cond_channels == 2
    assert net.in_channels == (4 if mode == "cat" else 3)
    ref = orc.param_shapes(X.cfg_of(mode))
    assert [(n, tuple(p.shape)) for n, p in net.named_parameters()] == [(n, tuple(s)) for n, s in ref]
    plan = net.plan                        # the HIP plan's own table agrees with the module's (checked on creation)
    assert plan.dx_mode == (L.DX_CAT if mode == "cat" else L.DX_ENC) and plan.dx_channels == 1 and plan.cond_channels == 2
    assert ("dx_enc.0.weight" in plan.param_names) == (mode == "enc")


def test_constructor_accepts_prob_and_refuses_the_rest():
    from mcedm_amd.ddim import PlCondDdim
    from tests import _ddpm_cond as D
    from tests.test_hip_module import wrap
    for mode in X.MODES:
        m = PlCondDdim(ddim_hparams(**X.model_update(mode)))
        assert m.dx_cond and m.dx_norm == "prob" and m.model.dx_cond and m.model.cat_dx == (mode == "cat")
        assert list(m.state_dict())[:2] == ["betas", "logvar"]
    for norm in ("l2", "gauss"):
        with pytest.raises(NotImplementedError, match="dx_cond with dx_norm"):
            PlCondDdim(ddim_hparams(dx_cond=True, dx_norm=norm))
    hp = D.hparams_dict()
    hp["model"].update(dx_cond=True, dx_norm="prob")
    with pytest.raises(NotImplementedError, match="dx_cond .* not built on the DDPM U-Net"):
        PlCondDdim(wrap(hp))
    assert not PlCondDdim(ddim_hparams()).dx_cond


def test_module_level_refusals():
    """What the guided path refuses, dx_cond refuses: checked on the helpers, which need no GPU for it."""
    import torch
    from mcedm_amd.ddim import PlCondDdim
    mk = lambda: PlCondDdim(ddim_hparams(**X.model_update("cat")))      # noqa: E731
    m = mk()
    z = torch.zeros(1, 32, 32, 1)
    sp = sparams(timesteps=5)
    for call in (lambda h: m.sample(h, z, sp), lambda h: m.sample_edm(h, z, m.sparams)):
        with pytest.raises(NotImplementedError, match="dx_cond .* on the device"):
            call(z)                                                          # h off the device
    with pytest.raises(NotImplementedError):
        m.sample(None, z, sp)
    on_device = types.SimpleNamespace(is_cuda=True, shape=(1, 32, 32, 1))
    assert PlCondDdim(ddim_hparams())._dx_input(None) is None
    m.pde_loss = None
    with pytest.raises(NotImplementedError, match="set_pde_loss_function"):
        m._dx_input(on_device)
    for attr, val in (("rescaled", True), ("normalization", "min_max"), ("h_ch", 2), ("u_ch", 2)):
        m = mk()
        m.set_pde_loss_function("swe_per", False)
        setattr(m, attr, val)
        with pytest.raises(NotImplementedError, match="scalar gauss-normalised"):
            m._dx_input(on_device)
        with pytest.raises(NotImplementedError, match="scalar gauss-normalised"):
            m._dx_train_input(z, z)
    m = mk()
    m.set_test_sampler_params(m.sparams)
    plain = PlCondDdim(ddim_hparams())
    plain.set_test_sampler_params(plain.sparams)
    with pytest.raises(NotImplementedError, match="without dx_cond"):
        plain.get_denoised(plain.model, z, 1.0, dx=z)


def dx_plan(mode="enc", in_channels=1):
    return L.Plan(in_channels, in_channels + 1, in_channels, 64, (1, 1, 1), 1, (32,), 128, dx_channels=in_channels,
                  dx_mode=L.DX_CAT if mode == "cat" else L.DX_ENC)


def _entries():
    dd = lambda cc=1: L.cond_ddim_desc(sparams(timesteps=5), alphas_ext(), cc, True)      # noqa: E731
    return [("mcedm_vp_heun_sample_dxcond", "vp_sampler_workspace_bytes", vp_desc),
            ("mcedm_cond_ddim_sample_dxcond", "cond_ddim_workspace_bytes", dd)]


def _call(entry, plan, sd, dxc, gd, cond=16, noise=None, seed=None, ws_bytes=1 << 40, hw=(R, R)):
    """A dx_cond sampler entry with dummy non-null pointers: every check below fails before a pointer is used."""
    p = lambda v: None if v is None else C.c_void_p(v)      # noqa: E731
    ref = lambda d: None if d is None else C.byref(d)       # noqa: E731
    outs = (p(16),) if "vp_heun" in entry else (p(16), p(16))
    rc = getattr(plan._lib, entry)(plan._h, p(16), C.byref(sd), ref(dxc), ref(gd), p(cond), p(16), p(noise), p(seed), *outs, 0, p(16),
                                   ws_bytes, Bq, *hw, None)
    return rc, plan._lib.mcedm_last_error().decode()


@pytest.mark.parametrize("mode", X.MODES)
@pytest.mark.parametrize("entry,query,mkdesc", _entries(), ids=[e[0] for e in _entries()])
def test_argument_checks_reject_on_the_host(entry, query, mkdesc, mode):
    plan, sd, dxc, gd = dx_plan(mode), mkdesc(), gdesc(), gdesc()
    plain = L.Plan(1, 2, 1, 64, (1, 1, 1), 1, (32,), 128)
    rc, msg = _call(entry, plain, sd, dxc, None)                           # not a dx_cond plan
    assert rc == -1 and "needs a dx_cond plan" in msg and "dx_mode 0" in msg, msg
    rc, msg = _call(entry, dx_plan(mode, 2), sd, dxc, None)                # two state / dx channels
    assert rc == -1 and "needs a dx_cond plan" in msg and "in_channels 2" in msg and "dx_channels 2" in msg, msg
    rc, msg = _call(entry, plan, sd, None, None)
    assert rc == -1 and "dxc" in msg and "is null" in msg, msg
    rc, msg = _call(entry, plan, sd, gdesc(3), None)
    assert rc == -1 and "dxc->system 3" in msg, msg
    rc, msg = _call(entry, plan, mkdesc(0), dxc, None, cond=None)
    assert rc == -1 and "dxc needs cond" in msg and "NULL" in msg, msg
    rc, msg = _call(entry, plan, mkdesc(0), dxc, None)                     # cond given, but the description says 0 channels
    assert rc == -1 and "dxc needs cond" in msg and "cond_channels 0" in msg, msg
    rc, msg = _call(entry, plan, sd, gdesc(2), None, hw=(32, 64))
    assert rc == -1 and "dxc: the Darcy residual needs a square grid" in msg, msg
    rc, msg = _call(entry, plan, sd, gdesc(2), None, hw=(4, 4))
    assert rc == -1 and "dxc: the Darcy residual needs a square grid" in msg, msg
    rc, msg = _call(entry, plan, sd, dxc, gdesc(3))                        # gd as guidance_check checks it
    assert rc == -1 and "gd->system 3" in msg, msg
    rc, msg = _call(entry, plan, sd, dxc, gdesc(2), hw=(32, 64))
    assert rc == -1 and "gd: the Darcy residual needs a square grid" in msg, msg
    rc, msg = _call(entry, plan, sd, dxc, gd, noise=16, seed=16)
    assert rc == -1 and "rng_seed are both given" in msg and ("step_noise" in msg or "eta_noise" in msg), msg
    # the workspace: exact with both descriptions, one gradient buffer [B, 1, H, W] fp32 less without guidance, and one (plus the
    # Darcy scratch, which the two share) more than the guided call of a plan without dx
    need = getattr(plan, query)(Bq, R, R, dxcond=True)
    grad = Bq * R * R * 4
    assert need == getattr(plan, query)(Bq, R, R, guided=True) + grad
    rc, msg = _call(entry, plan, sd, dxc, gd, ws_bytes=need - 1)
    assert rc == -3 and "workspace too small" in msg and str(need) in msg, msg
    rc, msg = _call(entry, plan, sd, dxc, None, ws_bytes=need - grad - 1)
    assert rc == -3 and "workspace too small" in msg and str(need - grad) in msg, msg


@pytest.mark.parametrize("mode", X.MODES)
def test_old_entries_keep_refusing_dx_plans(mode):
    plan = dx_plan(mode)
    p = lambda v: None if v is None else C.c_void_p(v)      # noqa: E731
    lib, vd, gd = plan._lib, vp_desc(), gdesc()
    dd = L.cond_ddim_desc(sparams(timesteps=5), alphas_ext(), 1, True)
    tail = (0, p(16), 1 << 40, Bq, R, R, None)
    calls = [lambda: lib.mcedm_vp_heun_sample(plan._h, p(16), C.byref(vd), p(16), p(16), None, p(16), *tail),
             lambda: lib.mcedm_vp_heun_sample_rng(plan._h, p(16), C.byref(vd), p(16), p(16), p(16), p(16), *tail),
             lambda: lib.mcedm_vp_heun_sample_guided(plan._h, p(16), C.byref(vd), C.byref(gd), p(16), p(16), None, None, p(16), *tail),
             lambda: lib.mcedm_cond_ddim_sample(plan._h, p(16), C.byref(dd), p(16), p(16), None, p(16), p(16), *tail),
             lambda: lib.mcedm_cond_ddim_sample_rng(plan._h, p(16), C.byref(dd), p(16), p(16), p(16), p(16), p(16), *tail),
             lambda: lib.mcedm_cond_ddim_sample_guided(plan._h, p(16), C.byref(dd), C.byref(gd), p(16), p(16), None, None, p(16), p(16),
                                                       *tail)]
    for call in calls:
        assert call() == -1 and "dx_cond plans are not supported" in lib.mcedm_last_error().decode()
    params = (C.c_void_p * len(plan.param_names))()
    rc = lib.mcedm_unet_backward_bucketed(plan._h, p(16), params, p(16), None, None, p(16), 1, p(16), params, p(16), 1 << 40, 1, R, R, 0,
                                          None, None, None)
    assert rc == -1 and "dx_cond plans go through" in lib.mcedm_last_error().decode()
    rc = lib.mcedm_unet_backward_dx(plan._h, p(16), params, p(16), None, None, None, p(16), 1, None, params, p(16), 1 << 40, 1, R, R, 0,
                                    None, None, None)
    assert rc == -1 and "null dF" in lib.mcedm_last_error().decode()


def test_binding_refuses_dx_input_where_no_entry_exists():
    from tests.test_cond_guided_cpu import ddpm_plan
    with pytest.raises(RuntimeError, match="dx_input .* is not built"):
        ddpm_plan()._sample_call("vp_sample", "mcedm_ddpm_vp_heun_sample", None, (), [], None, None, [], None, True, None, 0, (), "cpu",
                                 dx_input=gdesc())


@pytest.mark.parametrize("group", list(X.GOLDEN))
def test_fixtures_were_recorded_under_their_conditions(group):
    g = np.load(os.path.join(ROOT, "tests", "golden", X.GOLDEN[group]))
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", X.GOLDEN[group])) < 1000 * 1000 and int(g["seed"]) == X.SEED
    mode, guided = ("enc", True) if group == "guided" else (group, False)
    for tag in (X.GUIDED_TAGS if guided else X.SAMPLER_TAGS):
        key, S = X.sampler_key(mode, tag, guided), G.STEPS[tag]
        xs = g[f"{key}::xs"]
        assert xs.shape == (X.B, S + 1, X.H, X.W, 1) and np.isfinite(xs).all() and g[f"{key}::nodx_last"].shape == (X.B, 1, X.H, X.W, 1)
        if G.CASES[tag][0] == "sample":
            assert xs.dtype == np.float32 and g[f"{key}::x0_preds"].shape == (X.B, S, X.H, X.W, 1) and np.isfinite(g[f"{key}::x0_preds"]).all()
        else:
            assert xs.dtype == np.float64
        assert G.bars_apart(xs[:, -1], g[f"{key}::nodx_last"][:, 0]) == pytest.approx(float(g[f"{key}::moved_bars"]))
        if tag != "darcy":
            assert float(g[f"{key}::rerun_bars"]) <= 0.25 and float(g[f"{key}::moved_bars"]) >= 25.0
    for m in [m for m in X.MODES if X.TRAIN_FILE[m] == group]:
        assert float(g[f"{m}::train_moved_bars"]) >= 25.0
        n_params = len(orc.param_shapes(X.cfg_of(m)))
        for branch in X.BRANCHES:
            assert float(g[f"{m}::{branch}::rerun_bars"]) <= 0.5 and g[f"{m}::{branch}::grad_sqnorm_each"].shape == (n_params,)
            assert all(f"{m}::{branch}::grad::{n}" in g for n in X.grad_names(m))
    if group == "cat":
        assert int(g["dx_norm_l2_raises"]) == 1
    if not guided:
        assert all(g[f"{mode}::fwd_F_{k}"].shape == (4, 1, X.H, X.W) for k in ("sc_dx", "sc_nodx", "nosc_dx"))


def test_generator_reproduces_a_stored_case_bit_for_bit():
    ref = os.environ.get("MCEDM_REFERENCE", "/root/reference")
    if not os.path.isdir(os.path.join(ref, "models")):
        pytest.skip("the reference checkout is not on this machine")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_golden_cond_ddim_dx.py"), "--check", "cat::ddim_cfg_eta"],
                       capture_output=True, text=True)
    assert r.returncode == 0 and "bit-identical" in r.stdout, (r.stdout[-500:], r.stderr[-2000:])
