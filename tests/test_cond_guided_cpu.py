"""CPU checks of PlCondDdim's PDE guidance (guide_dx, reference models/ddim.py:1499-1503 and 1576-1590): the new entries in
header / library / binding, their host-side argument checks (they run before anything is enqueued), the guided workspace queries,
the conditions the fixture was recorded under and the module-level refusals."""
import ctypes as C
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import mcedm_amd  # noqa: F401
from mcedm_amd import lib as L
from tests import _cond_guided as G
from tests import _ddpm_cond as D
from tests.test_cond_ddim_cpu import ddim_hparams
from tests.test_cond_ddim_sample_cpu import alphas_ext, sparams
from tests.test_hip_module import wrap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mcedm_vp_guided_workspace_bytes", "mcedm_vp_heun_sample_guided", "mcedm_cond_ddim_guided_workspace_bytes",
       "mcedm_cond_ddim_sample_guided", "mcedm_ddpm_vp_guided_workspace_bytes", "mcedm_ddpm_vp_heun_sample_guided",
       "mcedm_ddpm_cond_ddim_guided_workspace_bytes", "mcedm_ddpm_cond_ddim_sample_guided", "mcedm_op_ddim_cond_step_guided"]
Bq, R = 3, 32


def test_new_entries_in_header_library_and_binding():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mcedm_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(mcedm_[a-z0-9_]+)\s*\(", src))
    nm = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (mcedm_[a-z0-9_]+)$", nm, flags=re.M))
    lib = L.load()
    L._bind_ops()
    for n in NEW:
        assert n in declared and n in L.EXPORTS + L.OP_EXPORTS and n in exported, n
        assert getattr(lib, n).argtypes, n
    assert lib.mcedm_version() == L.ABI_VERSION == 4
    assert set(L.GUIDED_ENTRIES.values()) == {n for n in NEW if "sample_guided" in n} and set(L.GUIDED_ENTRIES) <= set(L.SAMPLER_STEMS)
    # each guided entry takes the description and the seed pointer on top of its unguided stem
    for stem, guided in L.GUIDED_ENTRIES.items():
        assert len(getattr(lib, guided).argtypes) == len(getattr(lib, stem).argtypes) + 2, stem


def adm_plan(in_channels=1):
    return L.Plan(in_channels, in_channels + 1, in_channels, 64, (1, 1, 1), 1, (32,), 128)


def ddpm_plan(in_channels=1):
    return L.DdpmPlan(in_channels, in_channels, D.CFG.ch, D.CFG.ch_mult, D.CFG.num_res_blocks, D.CFG.attn_resolutions, R,
                      self_cond=True, cond_channels=1)


def vp_desc(cond_channels=1):
    return L.vp_sampler_desc(2, cond_channels, [2.0, 1.0, 0.0], [2.0, 1.0], [3.0, 2.0, 1.0, 0.0], 1.0, 0.0)


def gdesc(system=1):
    g = L.GuidanceDesc()
    g.system, g.weight = system, G.WEIGHT
    g.sub_h = g.sub_u = 0.0
    g.div_h = g.div_u = g.half_dt = g.dx = g.two_dx = 1.0
    return g


def _call(entry, plan, sd, gd, ddpm, cond=16, noise=None, seed=None, ws_bytes=1 << 40):
    """A guided sampler entry with dummy non-null pointers: every check below fails before a pointer is used."""
    p = lambda v: None if v is None else C.c_void_p(v)      # noqa: E731
    outs = (p(16),) if "vp_heun" in entry else (p(16), p(16))
    dims = (Bq,) if ddpm else (Bq, R, R)
    rc = getattr(plan._lib, entry)(plan._h, p(16), C.byref(sd), None if gd is None else C.byref(gd), p(cond), p(16), p(noise), p(seed),
                                   *outs, 0, p(16), ws_bytes, *dims, None)
    return rc, plan._lib.mcedm_last_error().decode()


def _entries():
    """(entry, size query, plan factory, sampler description factory, ddpm)"""
    dd = lambda cc=1: L.cond_ddim_desc(sparams(timesteps=5), alphas_ext(), cc, True)      # noqa: E731
    return [("mcedm_vp_heun_sample_guided", "vp_sampler_workspace_bytes", adm_plan, vp_desc, False),
            ("mcedm_cond_ddim_sample_guided", "cond_ddim_workspace_bytes", adm_plan, dd, False),
            ("mcedm_ddpm_vp_heun_sample_guided", "vp_sampler_workspace_bytes", ddpm_plan, vp_desc, True),
            ("mcedm_ddpm_cond_ddim_sample_guided", "cond_ddim_workspace_bytes", ddpm_plan, dd, True)]


@pytest.mark.parametrize("entry,query,mkplan,mkdesc,ddpm", _entries(), ids=[e[0] for e in _entries()])
def test_argument_checks_reject_on_the_host(entry, query, mkplan, mkdesc, ddpm):
    plan, sd, gd = mkplan(), mkdesc(), gdesc()
    rc, msg = _call(entry, mkplan(2), mkdesc(), gd, ddpm)                  # guidance on a 2-channel plan
    assert rc == -1 and "gd" in msg and "in_channels 2" in msg, msg
    rc, msg = _call(entry, plan, mkdesc(0), gd, ddpm, cond=None)           # guidance without the conditioning field
    assert rc == -1 and "gd needs cond" in msg and "NULL" in msg, msg
    rc, msg = _call(entry, plan, sd, gdesc(3), ddpm)
    assert rc == -1 and "gd->system 3" in msg, msg
    rc, msg = _call(entry, plan, sd, gd, ddpm, noise=16, seed=16)
    assert rc == -1 and "rng_seed are both given" in msg and ("step_noise" in msg or "eta_noise" in msg), msg
    rc, msg = _call(entry, plan, sd, None, ddpm, noise=16, seed=16)        # also without guidance
    assert rc == -1 and "rng_seed are both given" in msg, msg
    # the guided workspace is exact: what the unguided call needs plus the gradient and the Darcy scratch, [B, 1, H, W] fp32 each.
    # (mcedm_vp_sampler_workspace_bytes sizes its forward for B noise labels where the sampler uses one: an upper bound)
    plain, guided = getattr(plan, query)(Bq, R, R), getattr(plan, query)(Bq, R, R, guided=True)
    tight = guided - 2 * Bq * R * R * 4
    assert (plain >= tight if entry == "mcedm_vp_heun_sample_guided" else plain == tight) and guided >= plain
    rc, msg = _call(entry, plan, sd, gd, ddpm, ws_bytes=guided - 1)
    assert rc == -3 and "workspace too small" in msg and str(guided) in msg, msg
    rc, msg = _call(entry, plan, sd, None, ddpm, ws_bytes=tight - 1)       # gd NULL: the unguided size is what is asked for
    assert rc == -3 and "workspace too small" in msg and str(tight) in msg, msg


def test_darcy_guidance_needs_a_square_grid():
    plan = adm_plan()
    p = lambda v: C.c_void_p(v)      # noqa: E731
    gd, sd = gdesc(2), vp_desc()
    rc = plan._lib.mcedm_vp_heun_sample_guided(plan._h, p(16), C.byref(sd), C.byref(gd), p(16), p(16), None, None, p(16), 0, p(16), 1 << 40,
                                               Bq, 32, 64, None)
    assert rc == -1 and "Darcy residual needs a square grid" in plan._lib.mcedm_last_error().decode()


def test_step_op_rejects_dx_with_more_than_one_channel():
    lib = L._bind_ops()
    p = lambda v: None if v is None else C.c_void_p(v)      # noqa: E731
    common = (0.0, 1.0, 1.0, 1.0, 0.0, 1.0, p(16), None, None, 0, 0, 2, 2, 4, 4, None, 0, 0, None, 0, 0, None)
    rc = lib.mcedm_op_ddim_cond_step_guided(p(16), p(16), None, None, None, 0, p(16), 1.0, *common)
    assert rc == -1 and "C == 1" in L.load().mcedm_last_error().decode()
    rc = lib.mcedm_op_ddim_cond_step_guided(p(16), p(16), None, p(16), p(16), 0, None, 0.0, *common)
    assert rc == -1 and "both given" in L.load().mcedm_last_error().decode()


@pytest.mark.parametrize("net", G.NETS)
def test_fixture_was_recorded_under_its_conditions(net):
    g = np.load(os.path.join(ROOT, "tests", "golden", G.GOLDEN[net]))
    for tag in G.cases_of(net):
        key, S = f"{net}::{tag}", G.STEPS[tag]
        n = int(g[f"{key}::slots"])
        xs = g[f"{key}::xs"]
        assert G.MIN_SLOTS <= n <= S and xs.shape == (G.B, S + 1, G.H, G.W, 1)
        assert np.isfinite(xs[:, :n + 1]).all() and g[f"{key}::unguided_last"].shape == (G.B, 1, G.H, G.W, 1)
        if G.CASES[tag][0] == "sample":
            assert xs.dtype == np.float32 and g[f"{key}::x0_preds"].shape == (G.B, S, G.H, G.W, 1) and np.isfinite(g[f"{key}::x0_preds"][:, :n]).all()
        else:
            assert xs.dtype == np.float64
        if tag == "darcy":
            assert float(g[f"{key}::darcy_moved"]) == 0.0                  # the log-probability gradient saturates to exactly 0
            continue
        assert float(g[f"{key}::rerun_bars"]) <= 0.25 and float(g[f"{key}::moved_bars"]) >= 100.0
        assert G.bars_apart(xs[:, n], g[f"{key}::unguided_last"][:, 0]) == pytest.approx(float(g[f"{key}::moved_bars"]))


def test_generator_reproduces_a_stored_case_bit_for_bit():
    ref = os.environ.get("MCEDM_REFERENCE", "/root/reference")
    if not os.path.isdir(os.path.join(ref, "models")):
        pytest.skip("the reference checkout is not on this machine")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_golden_cond_guided.py"), "--check", "ddpm::ddim_cfg_eta"],
                       capture_output=True, text=True)
    assert r.returncode == 0 and "bit-identical" in r.stdout, (r.stdout[-500:], r.stderr[-2000:])


@pytest.mark.parametrize("net", G.NETS)
def test_module_level_refusals(net):
    from mcedm_amd.ddim import PlCondDdim
    z = torch.zeros(1, 32, 32, 1)
    mk = lambda: PlCondDdim(ddim_hparams() if net == "adm" else wrap(D.hparams_dict()))      # noqa: E731
    m = mk()
    sp = sparams(timesteps=5)
    for call in (lambda h: m.sample(h, z, sp, guide_dx=True), lambda h: m.sample_edm(h, z, m.sparams, guide_dx=True)):
        for h in (None, z):                                                # no conditioning field; tensors off the device
            with pytest.raises(NotImplementedError, match="guide_dx"):
                call(h)
    # the refusals PlCondEdm applies, reached with h on the device: checked on the helper, which needs no GPU for them
    on_device = types.SimpleNamespace(is_cuda=True, shape=(1, 32, 32, 1))
    assert m._guidance(None, False) is None
    for attr, val in (("rescaled", True), ("normalization", "min_max"), ("h_ch", 2), ("u_ch", 2)):
        m = mk()
        setattr(m, attr, val)
        with pytest.raises(NotImplementedError, match="scalar gauss-normalised"):
            m._guidance(on_device, True)
    m = mk()
    m.pde_loss = None
    with pytest.raises(NotImplementedError, match="set_pde_loss_function"):
        m._guidance(on_device, True)
