"""GPU: the DDPM U-Net executor (csrc/ddpm.hip) on every architecture of tests/_ddpm_arch.py -- widths 32 to 256, one to four
levels, one to three blocks per level, several attention blocks per level, both heads -- against the reference's own outputs
(tests/golden/ddpm_arch.npz, tools/make_golden_ddpm_arch.py) and against the fp64 oracle, both at the project's bar (rtol 1e-4,
atol 1e-5 max|ref|), with proof from the profiler rows that the intended path ran (the gn_coef_kernel table path or the fused
statistics; one attention launch per attention block), batch independence, repeatability on one workspace, and the Winograd /
input-resident kernel families switched off per plan."""
import collections
import functools

import pytest
import torch

from tests import _ddpm_arch as A
from tests import _knobs as K
from tests._ddpm_cond import check_cond_map

pytestmark = pytest.mark.gpu
B = A.B


@functools.lru_cache(maxsize=None)
def reference64(tag):
    """key -> the fp64 oracle's output, computed once per row."""
    P64 = A.params(tag, torch.float64)
    return {run[0]: A.oracle_forward(tag, P64, run) for run in A.runs(tag)}


def build(tag, **variants):
    import mcedm_amd  # noqa: F401
    from mcedm_amd import lib as L
    assert torch.cuda.is_available()
    cfg = A.ALL[tag]
    plan = A.make_plan(L, cfg)
    for which, value in variants.items():      # before the first use: conv_wino shapes the workspace
        plan.set_variant(which, value)
    P = A.params(tag)
    assert plan.param_names == [n for n, _ in A.ddo.param_shapes(cfg)]
    packed = plan.pack({k: v.cuda() for k, v in P.items()}, A.ddo.timestep_freqs(cfg.ch).cuda())
    return L, plan, packed


@functools.lru_cache(maxsize=None)
def net(tag):
    return build(tag)


def call(tag, plan, packed, run, ws=None, sample=None):
    """One stored run through the entry its plan has (forward / forward_cond on the map / forward_cat); sample: that one alone."""
    _, t, use_sc, use_cond = run
    cfg = A.ALL[tag]
    sel = (lambda v: v) if sample is None else (lambda v: v[sample:sample + 1].contiguous())
    x, xsc, cond = (None if v is None else sel(v).cuda() for v in A.inputs(tag))
    xsc, cond = xsc if use_sc else None, cond if use_cond else None
    if cfg.cat_cond:
        return plan.forward_cat(packed, x, t, cond=cond, ws=ws)
    if cfg.cond_channels:
        cmap = None if cond is None else plan.cond_map(packed, cond)
        return plan.forward_cond(packed, x, t, cond_map=cmap, x_self_cond=xsc, ws=ws)
    return plan.forward(packed, x, t, ws=ws, x_self_cond=xsc)


def held(got, key, golden_file, tag, what=""):
    """got against the golden and against the fp64 oracle, each at the bar; prints both ratios."""
    rg, r64 = A.bar_ratio(got, golden_file[key]), A.bar_ratio(got, reference64(tag)[key])
    print(f"{key}{what}: worst err / bar {rg:.4f} vs the reference's run, {r64:.4f} vs the fp64 oracle")
    assert got.dtype == torch.float32 and bool(torch.isfinite(got).all())
    assert rg <= 1.0 and r64 <= 1.0, (key, what, rg, r64)


# ---- 1. every row against the reference and the fp64 oracle ----------------------------------------------------------------------
@pytest.mark.parametrize("tag", list(A.ALL))
def test_forward_golden_and_fp64(golden, tag):
    """Both timesteps; a plain network with and without x_self_cond; the heads with cond given and None."""
    g = golden("ddpm_arch.npz")
    L, plan, packed = net(tag)
    for run in A.runs(tag):
        held(call(tag, plan, packed, run), run[0], g, tag)


# ---- 2. the intended path ran --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", list(A.ARCHS))
def test_the_intended_kernels_ran(tag):
    """gn_coef_kernel runs exactly on the rows where record_width leaves some GroupNorm without usable records (32- and
    96-channel tensors; the 192-channel concat of a quad- and a pair-record tensor, whose groups have 6 channels) and on no
    other row; launch_attention runs once per attention block of the configuration."""
    L, plan, packed = net(tag)
    run = A.runs(tag)[0]
    call(tag, plan, packed, run)               # anything lazily initialised settles outside the recording
    torch.cuda.synchronize()
    L.prof_enable(True)
    try:
        call(tag, plan, packed, run)
        torch.cuda.synchronize()
        report = L.prof_report()
    finally:
        L.prof_enable(False)
    rows = {r["name"]: r["launches"] for r in report}
    assert ("gn_coef_kernel" in rows) == A.TABLE_PATH[tag], (tag, sorted(rows))
    assert rows.get("attention_kernel", 0) == A.n_attention_blocks(A.ALL[tag]), (tag, rows.get("attention_kernel"))
    # ... each on the kernel its token count selects (the row's variants; tests/_knobs.py attn_fwd_variant)
    tokens = A.attention_tokens(A.ALL[tag])
    assert len(tokens) == A.n_attention_blocks(A.ALL[tag])
    want = dict(collections.Counter(K.attn_fwd_variant(T) for T in tokens))
    got = {r["name"]: r.get("variants") for r in report}.get("attention_kernel")
    assert got == want, (tag, got, want)
    if tag in A.SWITCHED:
        assert any(n.startswith("conv_wino") for n in rows), sorted(rows)


# ---- 3. batch independence, repeatability ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", list(A.ALL))
def test_sample_alone_and_second_call_are_bit_identical(tag):
    """Sample 1 of the B = 2 call == the B = 1 call on that sample (tile choices and the order of the statistics never depend on
    the batch size); a second call on the same workspace == the first."""
    L, plan, packed = net(tag)
    ws = L.Workspace()
    runs = A.runs(tag)
    run = runs[-1 if len(runs) == 2 else -2]      # t = 937, with x_self_cond / cond where the network takes one
    first = call(tag, plan, packed, run, ws=ws).clone()
    again = call(tag, plan, packed, run, ws=ws)
    assert torch.equal(first, again), float((first - again).abs().max())
    alone = call(tag, plan, packed, run, sample=1)
    assert torch.equal(alone[0], first[1]), float((alone[0] - first[1]).abs().max())


# ---- 4. kernel families switched off on this plan alone ----------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["conv_wino", "conv_resident"])
@pytest.mark.parametrize("tag", A.SWITCHED)
def test_kernel_family_switched_off_stays_within_the_bar(golden, tag, which):
    g = golden("ddpm_arch.npz")
    L, plan, packed = build(tag, **{which: 0})
    run = A.runs(tag)[0]
    L.prof_enable(True)
    try:
        got = call(tag, plan, packed, run)
        torch.cuda.synchronize()
        rows = sorted(r["name"] for r in L.prof_report())
    finally:
        L.prof_enable(False)
    assert not any(n.startswith(which) for n in rows), rows
    held(got, run[0], g, tag, what=f" [{which} = 0]")


# ---- 5. the map kernel of the head -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", list(A.HEADS))
def test_cond_map_against_the_formula_in_fp64(tag):
    """M = (Wc cond_enc.2) (*)circ GELU(cond_enc.0(cond)) + (Wx b_in + Wc b_enc2 + b_comb) in fp64 on the host, at ch = 32 with 3
    conditioning channels on 16 x 16 (one channel chunk, R below the kernel's 32-pixel block) and at 48 x 48 (a partial second
    block); interior, border ring (taken at the real R, where the wrap-around is read) and the four corners apart."""
    L, plan, packed = net(tag)
    cond = A.inputs(tag)[2]
    check_cond_map(plan.cond_map(packed, cond.cuda()), A.params(tag, torch.float64), cond, tag)
