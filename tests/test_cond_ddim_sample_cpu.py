"""CPU checks of the conditional DDIM sampler (PlCondDdim.sample, reference models/ddim.py:1452-1530): the C description built
from the reference's sampler parameters, the timestep sequences it walks, the new entries in header / library / binding, the
host-side argument checks of mcedm_cond_ddim_sample (they run before anything is enqueued) and PlCondEdm.sample, which keeps
raising."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import mcedm_amd  # noqa: F401
from mcedm_amd import lib as L
from tests.test_cond_ddim_cpu import ddim_hparams
from tests.test_hip_module import wrap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mcedm_cond_ddim_workspace_bytes", "mcedm_cond_ddim_sample", "mcedm_op_ddim_cond_step"]


def sparams(**over):
    """configs/diff_sampler/default.yaml: type ddim, 50 steps, uniform skipping, eta 0."""
    d = dict(name="ddim", type="ddim", timesteps=50, skip_type="uniform", eta=0.0, n_samples=1, n_repeat=1, n_time_h=0, n_time_u=0,
             return_last=True, select_by_pde=False, use_gt_pde_select=True, guide_dx=False, w=0.0, plot_scaled=False)
    d.update(over)
    return wrap(d)


def alphas_ext(n=1000):
    betas = torch.linspace(0.0001, 0.02, n, dtype=torch.float64).float()
    return (1 - torch.cat([torch.zeros(1), betas])).cumprod(dim=0)


def test_desc_helper_fields_and_dtypes():
    ae = alphas_ext()
    d = L.cond_ddim_desc(sparams(timesteps=10, skip_type="quad", eta=0.5, w=0.25), ae.double(), 1, True)
    assert isinstance(d, L.CondDdimDesc)
    assert (d.timesteps, d.skip_type, d.eta, d.w, d.cond_channels, d.self_cond, d.num_diffusion_timesteps) == (10, 1, 0.5, 0.25, 1, 1, 1000)
    assert [f for f, _ in L.CondDdimDesc._fields_] == ["timesteps", "skip_type", "eta", "w", "cond_channels", "self_cond",
                                                       "num_diffusion_timesteps", "alphas_cumprod_ext"]
    assert dict(L.CondDdimDesc._fields_)["eta"] is C.c_double and dict(L.CondDdimDesc._fields_)["timesteps"] is C.c_int32
    # the table travels as fp32 (the reference's compute_alpha works on the fp32 betas buffer) and is kept alive by the struct
    assert d._keep.dtype == torch.float32 and d._keep.numel() == 1001 and d._keep.is_contiguous()
    assert [d.alphas_cumprod_ext[i] for i in (0, 1, 1000)] == [float(ae[i]) for i in (0, 1, 1000)]
    d = L.cond_ddim_desc(sparams(w=None), ae, 2, False)
    assert (d.skip_type, d.w, d.cond_channels, d.self_cond) == (0, 0.0, 2, 0)


def test_desc_helper_rejects_an_unknown_skip_type():
    with pytest.raises(NotImplementedError, match="skip_type"):
        L.cond_ddim_desc(sparams(skip_type="cosine"), alphas_ext(), 1, True)


def test_ddim_timesteps_are_unchanged():
    """The sequence helper moved to a header the two samplers share: mcedm_ddim_timesteps returns what it returned."""
    for n in (100, 1000, 4000):
        for N in (1, 2, 7, 8, 10, 16, 50, 100):
            assert L.ddim_timesteps(n, N, "uniform") == list(range(0, n, n // N))
            assert L.ddim_timesteps(n, N, "quad") == [int(s) for s in list(np.linspace(0, np.sqrt(n * 0.8), N) ** 2)]
    assert L.ddim_timesteps(1000, 100, "quad")[-1] == 800 and L.ddim_timesteps(1000, 16, "quad")[1:4] == [3, 14, 31]
    assert len(L.ddim_timesteps(1000, 7, "uniform")) == 8                 # 1000 // 7 = 142: more entries than `timesteps`
    assert L.ddim_timesteps(1000, 8, "quad") == [0, 16, 65, 146, 261, 408, 587, 800]
    with pytest.raises(RuntimeError, match="bad schedule"):
        L.ddim_timesteps(10, 11, "quad")


def test_new_entries_declared_in_header_library_and_binding():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mcedm_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(mcedm_[a-z0-9_]+)\s*\(", src))
    lib = L.load()
    for n in NEW:
        assert n in declared and n in L.EXPORTS + L.OP_EXPORTS, n
        getattr(lib, n)
    assert "mcedm_cond_ddim_desc" in src and lib.mcedm_version() == L.ABI_VERSION == 4


def test_workspace_is_the_forward_plus_the_samplers_buffers():
    plan = L.Plan(1, 2, 1, 64, (1, 1, 1), 1, (32,), 128)
    B, H, W = 3, 32, 32
    n = B * H * W * 4
    own = 4 * n + 2 * 2 * n                      # xt, xt_next, F, F_uncond; cond' and its twin, two channels each
    # the forward inside the sampler carries one noise label for the batch: never more than the B-label forward's workspace
    assert own % 256 == 0 and own < plan.cond_ddim_workspace_bytes(B, H, W) <= plan.workspace_bytes(B, H, W) + own
    with pytest.raises(RuntimeError, match="multiples of 4"):
        plan.cond_ddim_workspace_bytes(1, 30, 32)


def _call(plan, d, cond=16, init=16, eta_noise=None, xs=16, x0=16, ws=16, ws_bytes=1 << 40, packed=16, desc=True):
    """mcedm_cond_ddim_sample with dummy non-null pointers: every check below fails before a pointer is used."""
    p = lambda v: None if v is None else C.c_void_p(v)
    rc = plan._lib.mcedm_cond_ddim_sample(plan._h, p(packed), C.byref(d) if desc else None, p(cond), p(init), p(eta_noise), p(xs),
                                          p(x0), 0, p(ws), ws_bytes, 3, 32, 32, None)
    return rc, plan._lib.mcedm_last_error().decode()


def test_argument_checks_reject_on_the_host():
    ae = alphas_ext()
    wide = L.Plan(1, 2, 1, 64, (1, 1, 1), 1, (32,), 128)                  # conditioning widened by the state channel
    plain = L.Plan(1, 1, 1, 64, (1, 1, 1), 1, (32,), 128)
    good = L.cond_ddim_desc(sparams(timesteps=10), ae, 1, True)
    for kw in (dict(packed=None), dict(desc=False), dict(init=None), dict(xs=None), dict(x0=None), dict(ws=None)):
        rc, msg = _call(wide, good, **kw)
        assert rc == -1 and "null argument" in msg, kw
    rc, msg = _call(L.Plan(2, 2, 1, 64, (1, 1, 1), 1, (32,), 128), good)
    assert rc == -1 and "in_channels != out_channels" in msg
    rc, msg = _call(L.Plan(1, 2, 1, 64, (1, 1, 1), 1, (32,), 128, dx_channels=1, dx_mode=L.DX_ENC), good)
    assert rc == -1 and "dx_cond plans" in msg
    for cc in (-1, 3):
        rc, msg = _call(wide, L.cond_ddim_desc(sparams(timesteps=10), ae, cc, False))
        assert rc == -1 and "cond_channels" in msg and "outside" in msg, cc
    rc, msg = _call(wide, good, cond=None)
    assert rc == -1 and "cond goes with cond_channels" in msg
    rc, msg = _call(plain, good)                                           # self_cond on a plan that is not widened
    assert rc == -1 and "not widened" in msg
    rc, msg = _call(wide, L.cond_ddim_desc(sparams(timesteps=10, eta=0.5), ae, 1, True))
    assert rc == -1 and "eta != 0 needs eta_noise" in msg
    rc, msg = _call(wide, L.cond_ddim_desc(sparams(timesteps=2000), ae, 1, True))
    assert rc == -1 and "bad schedule" in msg
    bad_skip = L.cond_ddim_desc(sparams(timesteps=10), ae, 1, True)
    bad_skip.skip_type = 2
    rc, msg = _call(wide, bad_skip)
    assert rc == -1 and "skip_type" in msg
    need = wide.cond_ddim_workspace_bytes(3, 32, 32)
    rc, msg = _call(wide, good, ws_bytes=need - 1)
    assert rc == -3 and "workspace too small" in msg and str(need) in msg


def test_plcondedm_sample_still_raises():
    from mcedm_amd.ddim import PlCondDdim, PlCondEdm
    from tests.test_hip_cond_edm import cond_hparams
    m = PlCondEdm(cond_hparams())
    with pytest.raises(NotImplementedError, match="Only EDM sampler is supported"):
        m.sample(torch.zeros(1, 32, 32, 1), torch.zeros(1, 32, 32, 1), sparams())
    assert "sample" in PlCondEdm.__dict__                                  # its own override, not PlCondDdim's loop
    d = PlCondDdim(ddim_hparams())
    with pytest.raises(NotImplementedError, match="guide_dx"):
        d.sample(torch.zeros(1, 32, 32, 1), torch.zeros(1, 32, 32, 1), sparams(), guide_dx=True)
