"""CPU checks of the DDPM U-Net on every architecture of tests/_ddpm_arch.py: the oracle against the reference's own outputs
(tests/golden/ddpm_arch.npz, written by tools/make_golden_ddpm_arch.py) in fp32 (bit for bit) and in fp64 (at the project's bar),
and the plan's parameter table against the oracle's -- names in ``Model.state_dict()`` order and shapes, which is the check on
the re-numbering of the up levels (built deepest first, registered level 0 first) where the levels differ in size."""
import pytest
import torch

import mcedm_amd  # noqa: F401
from mcedm_amd import lib as L
from tests import _ddpm_arch as A


@pytest.fixture
def generator_threads():
    """The thread count the golden was written with: the summation order of an fp32 CPU conv, and so its last bit, depends on it."""
    n = torch.get_num_threads()
    torch.set_num_threads(A.CPU_THREADS)
    yield
    torch.set_num_threads(n)


@pytest.mark.parametrize("tag", list(A.ALL))
def test_fp32_oracle_is_the_reference_bit_for_bit(golden, generator_threads, tag):
    g = golden("ddpm_arch.npz")
    P = A.params(tag)
    for run in A.runs(tag):
        y = A.oracle_forward(tag, P, run)
        assert y.dtype == torch.float32 and torch.equal(y, torch.as_tensor(g[run[0]])), run[0]


@pytest.mark.parametrize("tag", list(A.ALL))
def test_fp64_oracle_within_the_bar_of_the_reference(golden, tag):
    """The reference's fp32 rounding noise against the fp64 evaluation of the same formula sits far below the bar the HIP path is
    held to (rtol 1e-4, atol 1e-5 max|ref|)."""
    g = golden("ddpm_arch.npz")
    P64 = A.params(tag, torch.float64)
    worst = 0.0
    for run in A.runs(tag):
        y = A.oracle_forward(tag, P64, run)
        assert y.dtype == torch.float64
        worst = max(worst, A.bar_ratio(g[run[0]], y))
    print(f"{tag}: reference fp32 vs fp64 oracle, worst err / bar {worst:.4f}")
    assert worst <= 1.0, (tag, worst)


def test_every_stored_run_is_in_the_table(golden):
    g = golden("ddpm_arch.npz")
    assert sorted(k for k in g if k != "seed") == sorted(r[0] for tag in A.ALL for r in A.runs(tag)) and int(g["seed"]) == A.SEED


def test_the_table_reaches_what_it_claims():
    """The shapes the rows are there for, read off the oracle's parameter table: tensor widths, the number of bias rows of the
    timestep kernel (its grid is capped above 2048), attention blocks per row, up levels of unequal size."""
    def widths(tag):
        return {s[1] for n, s in A.ddo.param_shapes(A.ALL[tag]) if n.endswith(("conv1.weight", "nin_shortcut.weight"))}

    def bias_rows(tag):
        return sum(s[0] for n, s in A.ddo.param_shapes(A.ALL[tag]) if n.endswith("temb_proj.bias"))
    assert widths("narrow") == {32, 64, 96, 128} and widths("wide0") == {64, 128, 192} and {192, 256} <= widths("wide3")
    assert 256 in widths("rows3")               # 128 + 128, both from quad records (wide0 has no 256-channel concat: 64 + 128 twice)
    assert widths("nrb2") == widths("one") == widths("r48") == {64, 128}
    assert bias_rows("rows3") == 2816 and all(bias_rows(t) <= 2048 for t in A.ARCHS if t != "rows3")
    assert {t: A.n_attention_blocks(A.ARCHS[t]) for t in A.ARCHS} == dict(nrb2=11, one=4, r48=1, wide0=4, wide3=4, narrow=1, deep=6, rows3=1)
    per_level = [sum(n.startswith(f"up.{lv}.") for n, _ in A.ddo.param_shapes(A.ARCHS["deep"])) for lv in range(4)]
    assert len(set(per_level)) >= 3, per_level
    names = [n for n, _ in A.ddo.param_shapes(A.ARCHS["narrow"])]
    assert "down.1.block.0.nin_shortcut.weight" in names and "down.0.block.0.nin_shortcut.weight" not in names


@pytest.mark.parametrize("tag", list(A.ALL))
def test_plan_parameter_table_is_the_oracles(tag):
    """Plain, with the cond_enc head and with cat_cond: names in registration order, shapes, and the sizes a plan reports on the host."""
    cfg = A.ALL[tag]
    plan = A.make_plan(L, cfg)
    ref = A.ddo.param_shapes(cfg)
    assert plan.param_names == [n for n, _ in ref]
    assert plan.param_shapes == [tuple(s) for _, s in ref]
    assert len(set(plan.param_names)) == len(ref)
    assert plan.packed_bytes > 4 * sum(int(torch.tensor(s).prod()) for _, s in ref)
    assert plan.workspace_bytes(2) > plan.workspace_bytes(1) > 0
