"""GPU: the contract of the binding's one sampler call (lib._PlanBase._sample_call) and one graph wrapper (lib._GraphedCall),
for every sampler method on every plan kind that has it and for every Graphed* class:

  * materialised noise together with rng_seed, a malformed seed, a noise tensor one slot short and a wrong ``out`` are all
    rejected in Python, before anything is enqueued; a correct ``out`` is what comes back;
  * a replay equals the eager call on the same inputs bit for bit, with materialised and with device-side noise, also for the
    two wrappers built directly over a DdpmPlan with the cond_enc head; other inputs give another result;
  * ``seed`` goes with device-noise instances and only with them; an input's presence must be the captured one.

Shapes are the smallest at which these paths still differ: B = 2, 32 x 32, two sampler steps, n_repeat = 2."""
import pytest
import torch

from oracle import ddpm_oracle as dorc
from oracle import fixtures as fx
from oracle import mcedm_oracle as orc
from tests.test_cond_ddim_sample_cpu import alphas_ext, sparams
from tests.test_hip_cond_ddim import make_module
from tests.test_hip_ddpm_cond import make_module as make_ddpm_cond_module
from tests.test_hip_sampler_noise import _cond_edm_module, ddpm_net, dev_seed, L  # noqa: F401  (L, ddpm_net: fixtures)

pytestmark = pytest.mark.gpu
B, H, W, N, R = 2, 32, 32, 2, 2


class Case:
    """One sampler method on one plan.  call(noise, **kw) runs it with the materialised tensors of ``noise`` (name -> tensor;
    missing = None); spec: name -> (shape, dtype) of each; outs: the output shape(s) with return_last; inputs: the device
    tensors the method reads, in the order of the Graphed* call."""

    def __init__(self, method, call, spec, outs, inputs):
        self.method, self.call, self.spec, self.outs, self.inputs = method, call, spec, outs, inputs

    def noise(self, short=None):
        """Every materialised tensor at its right shape; ``short``: that one with one slot too few."""
        gen = torch.Generator().manual_seed(11)
        return {k: torch.rand(*((sh[0] - 1,) + sh[1:] if k == short else sh), generator=gen).to(dt).cuda()
                for k, (sh, dt) in self.spec.items()}


def _nchw(tag, C=1):
    return fx.randn(f"binding/{tag}", B, C, H, W).cuda()


def _vp_desc(lib):          # step 0 churns (t_hat > t_cur), step 1 does not
    return lib.vp_sampler_desc(N, 1, [20.0, 1.0, 0.0], [25.0, 1.0], [990.0, 900.0, 800.0, 0.0], 1.0, 0.0)


@pytest.fixture(scope="module")
def cases(L, golden, ddpm_net):
    """name -> Case.  The networks are the ones the sampler tests build; the modules are kept alive with the cases."""
    out, keep = {}, []
    step64 = lambda shape: {"step_noise": ((N,) + tuple(shape), torch.float64)}          # noqa: E731
    eta32 = lambda shape: {"eta_noise": ((N,) + tuple(shape), torch.float32)}            # noqa: E731
    sd = L.sampler_desc(orc.SamplerParams(timesteps=N, S_churn=15.0), 1.0, 0.002, 80.0)
    h, init = _nchw("h"), _nchw("init")
    with torch.no_grad():
        # Plan.sample and its guided / dx_cond forms: PlCondEdm's ADM network
        edm = {dx_cond: _cond_edm_module(golden, dx_cond) for dx_cond in (False, True)}
        for name, dx_cond, guided in (("sample", False, False), ("sample_guided", False, True), ("sample_dxcond", True, True)):
            m = edm[dx_cond]
            gd = m.pde_loss.guidance_desc(m.normalizer_input, m.normalizer_target, H, W)
            plan, pk = m.ema_model.ma_model.plan, m.ema_model.ma_model.packed_weights()
            kw0 = dict(guidance=gd if guided else None, dx_input=gd if dx_cond else None)
            out[name] = Case("sample", lambda nz, plan=plan, pk=pk, kw0=kw0, **kw: plan.sample(
                pk, sd, h, None, init, nz.get("step_noise"), **kw0, **kw), step64(init.shape), [(B, 1, H, W, 1)], (h, None, init))
            out[name].plan, out[name].pk, out[name].desc = plan, pk, sd
            keep.append(m)
        # vp_sample / cond_ddim_sample on both networks: PlCondDdim on the ADM U-Net and on the DDPM U-Net with the cond_enc head
        dd_tables = alphas_ext()
        for prefix, m in (("", make_module(golden)), ("ddpm_", make_ddpm_cond_module())):
            plan, pk = m.ema_model.ma_model.plan, m.ema_model.ma_model.packed_weights()
            vd = _vp_desc(L)
            dd = L.cond_ddim_desc(sparams(timesteps=N, eta=0.5), dd_tables, 1, True)
            assert len(L.ddim_timesteps(1000, N, "uniform")) == N
            out[prefix + "vp_sample"] = Case("vp_sample", lambda nz, plan=plan, pk=pk, vd=vd, **kw: plan.vp_sample(
                pk, vd, h, init, nz.get("step_noise"), **kw), step64(init.shape), [(B, 1, H, W, 1)], (h, init))
            out[prefix + "cond_ddim_sample"] = Case("cond_ddim_sample", lambda nz, plan=plan, pk=pk, dd=dd, **kw: plan.cond_ddim_sample(
                pk, dd, h, init, nz.get("eta_noise"), **kw), eta32(init.shape), [(B, 1, H, W, 1)] * 2, (h, init))
            for name, desc in (("vp_sample", vd), ("cond_ddim_sample", dd)):
                out[prefix + name].plan, out[prefix + name].pk, out[prefix + name].desc = plan, pk, desc
            keep.append(m)
        # the joint (h, u) DDPM: DDIM with RePaint loops, and RePaint
        plan, pk = ddpm_net
        cfg = fx.CFG_D
        S = cfg.resolution
        hu, init2 = fx.randn("binding/hu", B, 2, S, S).cuda(), fx.randn("binding/init2", B, 2, S, S).cuda()
        betas = dorc.betas_of(cfg)
        dd2, keep_dd = L.ddim_desc(dorc.DdimParams(timesteps=N, skip_type="uniform", eta=0.5, n_repeat=R, n_time_h=8, n_time_u=0),
                                   dorc.alphas_ext_of(betas), 1, 1, True)
        assert len(L.ddim_timesteps(cfg.num_timesteps, N, "uniform")) == N
        rd, keep_rd = L.repaint_desc(dorc.RepaintParams(timesteps=N, n_repeat=R, S_churn=15.0, n_time_h=8, n_time_u=0),
                                     dorc.edm_steps_of(betas), dorc.alphas_ext_of(betas), 1, 1)
        out["ddim_repaint_sample"] = Case("ddim_repaint_sample", lambda nz, **kw: plan.ddim_repaint_sample(
            pk, dd2, hu, init2, nz.get("eta_noise"), **kw), eta32(init2.shape), [(B, 1, S, S, 2)] * 2, (hu, init2))
        out["repaint_sample"] = Case("repaint_sample", lambda nz, **kw: plan.repaint_sample(
            pk, rd, hu, init2, nz.get("step_noise"), nz.get("repeat_noise"), **kw),
            {"step_noise": ((N,) + tuple(hu.shape), torch.float64), "repeat_noise": ((N, R - 1) + tuple(hu.shape), torch.float64)},
            [(B, 1, S, S, 2)], (hu, init2))
        for name, desc, k in (("ddim_repaint_sample", dd2, keep_dd), ("repaint_sample", rd, keep_rd)):
            out[name].plan, out[name].pk, out[name].desc, out[name].keep = plan, pk, desc, k
    out["_keep"] = keep
    return out


CASES = ["sample", "sample_guided", "sample_dxcond", "vp_sample", "ddpm_vp_sample", "cond_ddim_sample", "ddpm_cond_ddim_sample",
         "ddim_repaint_sample", "repaint_sample"]


# ---- the one sampler call -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_noise_and_seed_together_are_rejected(cases, name):
    c = cases[name]
    with pytest.raises(RuntimeError, match=f"{c.method}: .*not both"):
        c.call(c.noise(), rng_seed=dev_seed(1))
    for only in c.spec:                                   # one materialised tensor is enough
        with pytest.raises(RuntimeError, match="not both"):
            c.call({only: c.noise()[only]}, rng_seed=dev_seed(1))


@pytest.mark.parametrize("name", CASES)
def test_a_malformed_seed_is_rejected(cases, name):
    c = cases[name]
    for bad in (torch.ones(1, dtype=torch.int32, device="cuda"), torch.ones(2, dtype=torch.int64, device="cuda"),
                torch.ones(1, dtype=torch.int64)):                               # wrong dtype, two elements, on the host
        with pytest.raises(RuntimeError, match=f"{c.method}: rng_seed"):
            c.call({}, rng_seed=bad)


@pytest.mark.parametrize("name", CASES)
def test_a_noise_tensor_one_slot_short_is_rejected(cases, name):
    c = cases[name]
    for short in c.spec:
        with pytest.raises(RuntimeError, match=f"{c.method}: {short} must be"):
            c.call(c.noise(short=short))
    for wrong in c.spec:                                  # and so is the right shape in the wrong dtype
        nz = c.noise()
        nz[wrong] = nz[wrong].to(torch.float16)
        with pytest.raises(RuntimeError, match=f"{c.method}: {wrong} must be"):
            c.call(nz)


def _outs(c, shapes=None):
    dtype = torch.float32 if len(c.outs) == 2 else torch.float64
    ts = [torch.empty(sh, dtype=dtype, device="cuda") for sh in (shapes or c.outs)]
    return ts[0] if len(ts) == 1 else tuple(ts)


@pytest.mark.parametrize("name", CASES)
def test_out_is_checked_and_returned(cases, name):
    c = cases[name]
    wrong = [sh[:1] + (sh[1] + 1,) + sh[2:] for sh in c.outs]                    # a trajectory slot too many for return_last
    with pytest.raises(RuntimeError, match=f"{c.method}: out has shape"):
        c.call(c.noise(), out=_outs(c, wrong))
    if len(c.outs) == 2:                                                         # one of the pair wrong is wrong
        with pytest.raises(RuntimeError, match=f"{c.method}: out has shapes"):
            c.call(c.noise(), out=_outs(c, [c.outs[0], wrong[1]]))
    out = _outs(c)
    got = c.call(c.noise(), out=out)
    if len(c.outs) == 2:
        assert got[0] is out[0] and got[1] is out[1]
        assert all(bool(torch.isfinite(t).all()) for t in got)
    else:
        assert got is out and bool(torch.isfinite(got).all())
    fresh = c.call({}, rng_seed=dev_seed(5))                                     # without out: allocated at the same shapes
    assert [tuple(t.shape) for t in (fresh if len(c.outs) == 2 else (fresh,))] == c.outs


# ---- the one graph wrapper ------------------------------------------------------------------------------------------------
GRAPHED = ["GraphedSampler", "GraphedRepaint", "GraphedCondDdim", "GraphedDdimRepaint", "GraphedVpSampler",
           "ddpm:GraphedVpSampler", "ddpm:GraphedCondDdim"]
CASE_OF = {"GraphedSampler": "sample", "GraphedRepaint": "repaint_sample", "GraphedCondDdim": "cond_ddim_sample",
           "GraphedDdimRepaint": "ddim_repaint_sample", "GraphedVpSampler": "vp_sample", "ddpm:GraphedVpSampler": "ddpm_vp_sample",
           "ddpm:GraphedCondDdim": "ddpm_cond_ddim_sample"}


def _build(L, cases, which, device_noise, has_cond=True):
    c = cases[CASE_OF[which]]
    cls = which.split(":")[-1]
    if cls == "GraphedSampler":
        return L.GraphedSampler(c.plan, c.pk, c.desc, B, H, W, masked=False, has_cond=has_cond, churn=True, device_noise=device_noise)
    if cls == "GraphedRepaint":
        return L.GraphedRepaint(c.plan, c.pk, c.desc, c.keep, B)
    if cls == "GraphedCondDdim":
        return L.GraphedCondDdim(c.plan, c.pk, c.desc, B, H, W, stochastic=True, device_noise=device_noise)
    if cls == "GraphedDdimRepaint":
        return L.GraphedDdimRepaint(c.plan, c.pk, c.desc, c.keep, B, stochastic=True, device_noise=device_noise)
    return L.GraphedVpSampler(c.plan, c.pk, c.desc, B, H, W, has_cond=has_cond, churn=True, device_noise=device_noise)


@pytest.fixture(scope="module")
def graphed(L, cases):
    """(class, device_noise) -> the captured instance, built on first use and shared by the tests below."""
    made = {}

    def get(which, device_noise):
        device_noise = device_noise or which == "GraphedRepaint"                 # RePaint replays with device-side noise only
        if (which, device_noise) not in made:
            with torch.no_grad():
                made[which, device_noise] = _build(L, cases, which, device_noise)
        return made[which, device_noise]
    return get


def _clone(t):
    return tuple(x.clone() for x in t) if isinstance(t, tuple) else t.clone()


def _equal(a, b):
    a, b = (a if isinstance(a, tuple) else (a,)), (b if isinstance(b, tuple) else (b,))
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("device_noise", [False, True])
@pytest.mark.parametrize("which", GRAPHED)
def test_replay_equals_the_eager_call(cases, graphed, which, device_noise):
    if which == "GraphedRepaint" and not device_noise:
        return                                                                    # no such instance: its noise is device-side
    c, g = cases[CASE_OF[which]], graphed(which, device_noise)
    assert (g.seed is not None) == device_noise and g.graph is not None and g.ws is not None
    nz = c.noise()
    args = c.inputs + (() if device_noise else tuple(nz.values()))
    kw, kw2 = (dict(seed=77), dict(seed=78)) if device_noise else ({}, {})
    with torch.no_grad():
        eager = c.call({}, rng_seed=dev_seed(77)) if device_noise else c.call(nz)
        first, again = _clone(g(*args, **kw)), _clone(g(*args, **kw))
        if device_noise:
            assert _equal(_clone(g(*args, seed=dev_seed(77))), first)            # the seed as a tensor
            other = _clone(g(*args, **kw2))                                      # other draws
        else:
            other = _clone(g(*[t if t is None else t + 1 for t in c.inputs], *nz.values()))      # other inputs, same draws
        assert g(*args, **kw) is g.out                                           # the instance's static output
    assert _equal(first, eager), "replay and eager launches differ"
    assert _equal(again, first) and not _equal(other, first)
    assert all(bool(torch.isfinite(t).all()) for t in (other if isinstance(other, tuple) else (other,)))


@pytest.mark.parametrize("which", GRAPHED)
def test_seed_goes_with_device_noise_instances_only(cases, graphed, which):
    c = cases[CASE_OF[which]]
    noise = list(c.noise().values())
    if which == "GraphedRepaint":
        with pytest.raises(RuntimeError, match="GraphedRepaint: 'seed'"):
            graphed(which, True)(*c.inputs, None)
        return
    cls = which.split(":")[-1]
    with pytest.raises(RuntimeError, match=f"{cls}: 'seed'"):
        graphed(which, False)(*c.inputs, *noise, seed=3)
    with pytest.raises(RuntimeError, match=f"{cls}: 'seed'"):
        graphed(which, True)(*c.inputs)


@pytest.mark.parametrize("which", GRAPHED)
def test_an_input_must_be_present_exactly_when_it_was_captured(L, cases, graphed, which):
    c = cases[CASE_OF[which]]
    cls = which.split(":")[-1]
    seed = (7,) if which == "GraphedRepaint" else ()
    kw = {} if which == "GraphedRepaint" else dict(seed=7)
    g = graphed(which, True)
    first = "hu" if "Repaint" in cls else "cond"
    with pytest.raises(RuntimeError, match=f"{cls}: '{first}' presence differs"):              # captured with, called without
        g(None, *c.inputs[1:], *seed, **kw)
    with pytest.raises(RuntimeError, match=f"{cls}: 'init_noise' presence differs"):
        g(*c.inputs[:-1], None, *seed, **kw)
    # captured without, called with
    if cls == "GraphedSampler":
        with pytest.raises(RuntimeError, match="GraphedSampler: 'mask' presence differs"):
            g(c.inputs[0], torch.ones_like(c.inputs[2]), c.inputs[2], **kw)
    if which == "GraphedVpSampler":                                               # (the DDPM entry ties cond to the description)
        with torch.no_grad():
            bare = _build(L, cases, which, True, has_cond=False)
        assert bare.cond is None
        with pytest.raises(RuntimeError, match=f"{cls}: 'cond' presence differs"):
            bare(*c.inputs, **kw)
        assert bool(torch.isfinite(bare(None, c.inputs[1], **kw)).all())
    if which != "GraphedRepaint":                                                 # the noise buffer of a device-noise instance
        name, t = next(iter(c.noise().items()))
        with pytest.raises(RuntimeError, match=f"{cls}: '{name}' presence differs"):
            g(*c.inputs, t, **kw)
