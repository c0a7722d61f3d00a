"""CPU checks of the device-side noise of the remaining samplers: the new entries in header / library / binding, the host-side
argument checks of every `_rng` entry (a null seed, then the sibling entry's own checks; all run before anything is enqueued)
and the `noise_source` attribute of the two single-task modules."""
import ctypes as C
import os
import re

import mcedm_amd  # noqa: F401
from mcedm_amd import lib as L
from oracle import mcedm_oracle as orc
from tests.test_cond_ddim_sample_cpu import alphas_ext, sparams

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mcedm_uniform_fill", "mcedm_cond_ddim_sample_rng", "mcedm_ddim_repaint_sample_rng", "mcedm_heun_sample_guided_rng",
       "mcedm_heun_sample_dxcond_rng", "mcedm_op_ddim_cond_step_rng"]
ONE = 16                       # a dummy non-null pointer: every check below fails before a pointer is used


def p(v):
    return None if v is None else C.c_void_p(v)


def err(lib):
    return lib.mcedm_last_error().decode()


def test_new_entries_declared_in_header_library_and_binding():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mcedm_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(mcedm_[a-z0-9_]+)\s*\(", src))
    lib = L._bind_ops()
    for n in NEW:
        assert n in declared and n in L.EXPORTS + L.OP_EXPORTS, n
        assert getattr(lib, n).argtypes, n                                 # bound, with its argument types
    assert lib.mcedm_version() == L.ABI_VERSION == 4
    for name in ("uniform_fill", "GraphedDdimRepaint", "GraphedVpSampler"):
        assert hasattr(L, name), name


def _cond_ddim_rng(plan, d, seed=ONE, cond=ONE, ws_bytes=1 << 40):
    rc = plan._lib.mcedm_cond_ddim_sample_rng(plan._h, p(ONE), C.byref(d), p(cond), p(ONE), p(seed), p(ONE), p(ONE), 0, p(ONE),
                                              ws_bytes, 3, 32, 32, None)
    return rc, err(plan._lib)


def test_cond_ddim_sample_rng_checks():
    ae = alphas_ext()
    wide = L.Plan(1, 2, 1, 64, (1, 1, 1), 1, (32,), 128)
    good = L.cond_ddim_desc(sparams(timesteps=10, eta=0.5), ae, 1, True)
    rc, msg = _cond_ddim_rng(wide, good, seed=None)
    assert rc == -1 and "rng_seed" in msg
    need = wide.cond_ddim_workspace_bytes(3, 32, 32)
    rc, msg = _cond_ddim_rng(wide, good, ws_bytes=need - 1)
    assert rc == -3 and "workspace too small" in msg and str(need) in msg
    dxp = L.Plan(1, 2, 1, 64, (1, 1, 1), 1, (32,), 128, dx_channels=1, dx_mode=L.DX_ENC)
    rc, msg = _cond_ddim_rng(dxp, good)
    assert rc == -1 and "dx_cond plans" in msg
    for cc in (-1, 3):
        rc, msg = _cond_ddim_rng(wide, L.cond_ddim_desc(sparams(timesteps=10), ae, cc, False))
        assert rc == -1 and "cond_channels" in msg and "outside" in msg, cc
    rc, msg = _cond_ddim_rng(wide, good, cond=None)
    assert rc == -1 and "cond goes with cond_channels" in msg


def _ddpm_plan():
    from oracle import fixtures as fx
    cfg = fx.CFG_D
    return L.DdpmPlan(cfg.in_channels, cfg.out_ch, cfg.ch, cfg.ch_mult, cfg.num_res_blocks, cfg.attn_resolutions, cfg.resolution)


def _ddim_repaint_rng(plan, d, seed=ONE, ws_bytes=1 << 40, hu=ONE):
    rc = plan._lib.mcedm_ddim_repaint_sample_rng(plan._h, p(ONE), C.byref(d), p(hu), p(ONE), p(seed), p(ONE), p(ONE), 0, p(ONE),
                                                 ws_bytes, 2, None)
    return rc, err(plan._lib)


def test_ddim_repaint_sample_rng_checks():
    from oracle import ddpm_oracle as dorc
    plan = _ddpm_plan()
    ae = alphas_ext()
    sp = dorc.DdimParams(timesteps=4, skip_type="quad", eta=0.01, n_repeat=3, n_time_h=8, n_time_u=0)
    d, keep = L.ddim_desc(sp, ae, 1, 1, True)
    rc, msg = _ddim_repaint_rng(plan, d, seed=None)
    assert rc == -1 and "rng_seed" in msg
    need = plan.ddim_workspace_bytes(2)
    rc, msg = _ddim_repaint_rng(plan, d, ws_bytes=need - 1)
    assert rc == -3 and "workspace too small" in msg and str(need) in msg
    rc, msg = _ddim_repaint_rng(plan, d, hu=None)
    assert rc == -1 and "null argument" in msg
    bad, keep2 = L.ddim_desc(sp, ae, 2, 1, True)
    rc, msg = _ddim_repaint_rng(plan, bad)
    assert rc == -1 and "h_ch + u_ch" in msg
    bad_skip, keep3 = L.ddim_desc(sp, ae, 1, 1, True)
    bad_skip.skip_type = 2
    rc, msg = _ddim_repaint_rng(plan, bad_skip)
    assert rc == -1 and "skip_type" in msg


def test_guided_and_dxcond_rng_checks():
    lib = L.load()
    plain = L.Plan(1, 1, 1, 64, (1, 1, 1), 1, (32,), 128)
    dxp = L.Plan(1, 1, 1, 64, (1, 1, 1), 1, (32,), 128, dx_channels=1, dx_mode=L.DX_ENC)
    sd = L.sampler_desc(orc.SamplerParams(timesteps=4, S_churn=15.0))
    gd = L.GuidanceDesc(1, 0.002, 0.03125, 0.0, 0.0, 1.0, 0.0, 1.0, 5.0)
    bad_gd = L.GuidanceDesc(3, 0.002, 0.03125, 0.0, 0.0, 1.0, 0.0, 1.0, 5.0)

    def guided(plan, g, seed=ONE, mask=None, ws_bytes=1 << 40):
        rc = lib.mcedm_heun_sample_guided_rng(plan._h, p(ONE), C.byref(sd), C.byref(g), p(ONE), p(mask), p(ONE), p(seed), p(ONE), 1,
                                              p(ONE), ws_bytes, 3, 32, 32, None)
        return rc, err(lib)

    def dxcond(plan, g, seed=ONE, ws_bytes=1 << 40):
        rc = lib.mcedm_heun_sample_dxcond_rng(plan._h, p(ONE), C.byref(sd), C.byref(g), None, p(ONE), p(ONE), p(seed), p(ONE), 1,
                                              p(ONE), ws_bytes, 3, 32, 32, None)
        return rc, err(lib)
    rc, msg = guided(plain, gd, seed=None)
    assert rc == -1 and "rng_seed" in msg
    rc, msg = guided(plain, bad_gd)
    assert rc == -1 and "guidance system must be 1 (SWE) or 2 (Darcy)" in msg
    rc, msg = guided(plain, gd, mask=ONE)
    assert rc == -1 and "PDE guidance is defined for the single-task sampler" in msg
    # (mcedm_sampler_workspace_bytes sizes the network for one noise level per sample, the sampler needs one for the batch: the
    # entry's own threshold lies below the query, so the check is exercised with a buffer that is short by any count)
    rc, msg = guided(plain, gd, ws_bytes=plain.sampler_workspace_bytes(3, 32, 32) // 2)
    assert rc == -3 and "workspace too small" in msg
    rc, msg = dxcond(dxp, gd, seed=None)
    assert rc == -1 and "rng_seed" in msg
    rc, msg = dxcond(plain, gd)
    assert rc == -1 and "dx_cond plan" in msg
    rc, msg = dxcond(dxp, bad_gd)
    assert rc == -1 and "dx system must be 1 (SWE) or 2 (Darcy)" in msg
    rc, msg = dxcond(dxp, gd, ws_bytes=dxp.sampler_workspace_bytes(3, 32, 32) // 2)
    assert rc == -3 and "workspace too small" in msg


def test_uniform_fill_and_step_op_reject_a_null_seed():
    lib = L._bind_ops()
    assert lib.mcedm_uniform_fill(p(ONE), 4, None, 0, None) == -1 and "null argument" in err(lib)
    assert lib.mcedm_uniform_fill(None, 4, p(ONE), 0, None) == -1
    rc = lib.mcedm_op_ddim_cond_step_rng(p(ONE), p(ONE), None, None, 0, 0.0, 1.0, 1.0, 1.0, 0.5, 0.5, p(ONE), None, None, 0, 0, 1, 1, 4, 4,
                                         None, 0, 0, None, 0, 0, None)
    assert rc == -1 and "rng_seed" in err(lib)


def test_single_task_modules_read_the_noise_source_from_the_environment(monkeypatch):
    from mcedm_amd.ddim import PlCondDdim, PlCondEdm
    from tests.test_cond_ddim_cpu import ddim_hparams
    from tests.test_hip_cond_edm import cond_hparams
    monkeypatch.delenv("MCEDM_NOISE_SOURCE", raising=False)
    assert PlCondEdm(cond_hparams()).noise_source == PlCondDdim(ddim_hparams()).noise_source == "device"
    monkeypatch.setenv("MCEDM_NOISE_SOURCE", "torch")
    assert PlCondEdm(cond_hparams()).noise_source == PlCondDdim(ddim_hparams()).noise_source == "torch"


def test_every_sampler_stem_has_an_rng_twin_in_header_library_and_binding():
    """lib.SAMPLER_STEMS is what _PlanBase._sample_call dispatches on: each stem and its `_rng` twin is exported, declared and
    bound, and the twin takes ONE seed pointer where the stem takes its materialised-noise pointers."""
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mcedm_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(mcedm_[a-z0-9_]+)\s*\(", src))
    lib = L.load()
    for stem, n_noise in L.SAMPLER_STEMS.items():
        for name in (stem, stem + "_rng"):
            assert name in L.EXPORTS and name in declared, name
            assert getattr(lib, name).argtypes, name
        assert n_noise >= 1
        assert len(getattr(lib, stem + "_rng").argtypes) == len(getattr(lib, stem).argtypes) - (n_noise - 1), stem
    # and the table is complete: every exported `_rng` sampler entry is the twin of a row
    assert {n[:-len("_rng")] for n in L.EXPORTS if n.endswith("_rng")} == set(L.SAMPLER_STEMS)


def test_desc_key():
    sp = orc.SamplerParams(timesteps=4, S_churn=15.0)
    a, b = L.sampler_desc(sp), L.sampler_desc(sp)
    assert L.desc_key(a) == L.desc_key(b) and hash(L.desc_key(a)) == hash(L.desc_key(b))
    assert len(L.desc_key(a)) == len(L.SamplerDesc._fields_)
    b.S_churn = 14.0
    assert L.desc_key(a) != L.desc_key(b)
    ae = alphas_ext()
    d = L.cond_ddim_desc(sparams(timesteps=10, eta=0.5), ae, 1, True)
    e = L.cond_ddim_desc(sparams(timesteps=10, eta=0.5), ae.clone(), 1, True)           # another table at another address
    key = L.desc_key(d, skip=("alphas_cumprod_ext",))
    assert key == L.desc_key(e, skip=("alphas_cumprod_ext",)) == (10, 0, 0.5, 0.0, 1, 1, 1000)
    assert len(key) == len(L.CondDdimDesc._fields_) - 1 and not any(isinstance(v, C._Pointer) for v in key)
    e.eta = 0.25
    assert L.desc_key(e, skip=("alphas_cumprod_ext",)) != key
    from oracle import ddpm_oracle as dorc
    rp = dorc.RepaintParams(timesteps=4, n_repeat=2, S_churn=0.0, n_time_h=0, n_time_u=16)
    from oracle import fixtures as fx
    betas = dorc.betas_of(fx.CFG_D)
    rd, keep = L.repaint_desc(rp, dorc.edm_steps_of(betas), dorc.alphas_ext_of(betas), 1, 1)
    rkey = L.desc_key(rd, skip=("edm_steps", "alphas_cumprod_ext"))
    assert len(rkey) == len(L.RepaintDesc._fields_) - 2 and not any(isinstance(v, C._Pointer) for v in rkey)
    hash(rkey)
