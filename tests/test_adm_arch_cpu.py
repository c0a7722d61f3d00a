"""CPU checks of the ADM U-Net on every architecture of tests/_adm_arch.py: the oracle against the reference's own outputs
(tests/golden/adm_arch.npz, written by tools/make_golden_adm_arch.py) in fp32 (bit for bit) and in fp64 (forward, loss and
gradients at the project's bar), the plan's parameter table and workspace sizes against the oracle's table, and the shapes
each row of the table is there for."""
import functools

import numpy as np
import pytest
import torch

import mcedm_amd  # noqa: F401
from mcedm_amd import lib as L
from tests import _adm_arch as A
from tests import _attn_bwd as AB


@pytest.fixture
def generator_threads():
    """The thread count the golden was written with: the summation order of an fp32 CPU conv, and so its last bit, depends on it."""
    n = torch.get_num_threads()
    torch.set_num_threads(A.CPU_THREADS)
    yield
    torch.set_num_threads(n)


@pytest.mark.parametrize("tag", list(A.ARCHS))
def test_fp32_oracle_is_the_reference_bit_for_bit(golden, generator_threads, tag):
    g = golden("adm_arch.npz")
    P = A.params(tag)
    for key, kind in A.runs(tag):
        F = A.denoise_ref(tag, P, kind)[1]
        assert F.dtype == torch.float32 and torch.equal(F, torch.as_tensor(g[key])), key


@pytest.mark.parametrize("tag", list(A.ARCHS))
def test_fp64_forward_within_the_bar_of_the_reference(golden, tag):
    """The reference's fp32 rounding noise against the fp64 evaluation of the same formula sits far below the bar the HIP path is
    held to (rtol 1e-4, atol 1e-5 max|ref|)."""
    g = golden("adm_arch.npz")
    P64 = A.params(tag, torch.float64)
    worst = 0.0
    for key, kind in A.runs(tag):
        F = A.denoise_ref(tag, P64, kind)[1]
        assert F.dtype == torch.float64
        worst = max(worst, A.bar_ratio(g[key], F))
    print(f"{tag}: reference fp32 vs fp64 oracle, forward, worst err / bar {worst:.4f}")
    assert worst <= 1.0, (tag, worst)


@pytest.mark.parametrize("tag", list(A.ARCHS))
def test_fp64_training_step_within_the_bar_of_the_reference(golden, tag):
    """Loss, the three stored gradients and every parameter's squared gradient norm: fp64 autograd through the oracle against the
    reference network's own fp32 autograd.  A squared norm moves by twice the relative error of its tensor, hence 2e-4 (+ the
    atol share, 2e-5, for a tensor whose entries all sit far below its maximum)."""
    g = golden("adm_arch.npz")
    loss, grads = A.training_grads(tag)
    r_loss = A.bar_ratio(g[f"{tag}::loss"].reshape(1), loss.reshape(1))
    r = {n: A.bar_ratio(g[f"{tag}::grad::{n}"], grads[n]) for n in A.grad_names(tag)}
    print(f"{tag}: reference fp32 vs fp64 oracle, loss {r_loss:.4f}, stored gradients {max(r.values()):.4f}")
    assert r_loss <= 1.0 and max(r.values()) <= 1.0, (tag, r_loss, r)
    each = np.array([float((v ** 2).sum()) for v in grads.values()])
    np.testing.assert_allclose(g[f"{tag}::grad_sqnorm_each"], each, rtol=2.2e-4)


def test_every_stored_key_is_in_the_table(golden):
    g = golden("adm_arch.npz")
    assert sorted(k for k in g if k != "seed") == sorted(k for tag in A.ARCHS for k in A.golden_keys(tag)) and int(g["seed"]) == A.SEED


@functools.lru_cache(maxsize=None)
def plan_of(tag):
    return A.make_plan(L, A.cfg_of(tag))


@pytest.mark.parametrize("tag", list(A.ARCHS))
def test_plan_parameter_table_and_workspace(tag):
    """Names in state_dict() order and shapes; the workspace is positive and grows with the batch and with training."""
    cfg, B, H, W = A.ARCHS[tag]
    plan = plan_of(tag)
    ref = A.orc.param_shapes(cfg)
    assert plan.param_names == [n for n, _ in ref]
    assert plan.param_shapes == [tuple(s) for _, s in ref]
    assert len(set(plan.param_names)) == len(ref)
    assert plan.packed_bytes > 4 * sum(int(np.prod(s)) for _, s in ref)
    assert plan.workspace_bytes(B + 1, H, W) > plan.workspace_bytes(B, H, W) > 0
    assert plan.workspace_bytes(B, H, W, True) > plan.workspace_bytes(B, H, W)
    assert plan.workspace_bytes(B + 1, H, W, True) > plan.workspace_bytes(B, H, W, True)
    if len(cfg.ch_mult) > 1:
        with pytest.raises(RuntimeError, match="multiples of"):
            plan.workspace_bytes(B, H + 1, W)


def test_the_table_reaches_what_it_claims():
    """The shapes the rows are there for, read off the oracle's parameter table and the level sizes."""
    cpg = {t: A.gn_widths(t) for t in A.ARCHS}
    assert cpg["one"] == {64: 4, 128: 4} and cpg["c128a"] == {128: 4, 256: 8}
    assert cpg["rect"] == {64: 4, 128: 4, 192: 6, 256: 8}
    assert cpg["ragged"] == {64: 4, 128: 4, 192: 6, 256: 8}
    assert cpg["narrow"] == {40: 4, 80: 4, 120: 4, 160: 5}
    assert cpg["ch24"] == {24: 4, 48: 4, 72: 4, 96: 4}
    assert cpg["wide3"] == {64: 4, 128: 4, 192: 6, 256: 8, 384: 12}
    assert cpg["deep"] == {32: 4, 64: 4, 96: 4, 128: 4, 192: 6, 256: 8}
    assert cpg["nrb3"] == {64: 4, 128: 4, 192: 6, 256: 8}
    assert cpg["c192"] == {192: 6, 384: 12}
    assert cpg["attn_rag"] == {64: 4, 128: 4, 192: 6, 256: 8}
    # the ADM executor's statistics records hold 4 channels: a row needs the full-pass table exactly where some group is not whole records
    assert {t: any(v % 4 for v in cpg[t].values()) for t in A.ARCHS} == {t: A.PATHS[t]["table"] for t in A.ARCHS}
    # attention blocks and their token counts
    # (narrow and ch24 have none: their deepest level is narrower than one head, and dec.*_in0 then has no attention, adm_blocks.py:135)
    tokens = {t: sorted(A.attention_tokens(t)) for t in A.ARCHS}
    assert tokens == dict(one=[64] * 4, rect=[384], ragged=[15] * 4, narrow=[], ch24=[], wide3=[256] * 4, deep=[4] + [16] * 5,
                          nrb3=[128] + [512] * 7, c192=[1024] * 4, c128a=[256] * 4 + [1024] * 3, attn_rag=[100] * 4 + [400] * 3)
    assert {4, 15, 16, 100, 128, 256, 400, 512, 1024} <= {n for v in tokens.values() for n in v}
    # every branch of the attention backward (tests/_attn_bwd.py) in some training step
    assert {AB.branch(n) for v in tokens.values() for n in v} == {"direct<1>", "direct<2>", "direct<4>", "lds"}
    assert sorted(AB.branch(n) for n in tokens["attn_rag"]) == ["direct<2>"] * 4 + ["direct<4>"] * 3
    for t in A.ARCHS:
        assert len(tokens[t]) == sum(n.endswith(".qkv.weight") for n, _ in A.orc.param_shapes(A.cfg_of(t)))
    # a level on whole 8 x 16 tiles with at least 1024 pixels and a width the large Winograd kernel serves (Cout % 64 == 0) ...
    big = {t: [(h, w, c) for h, w, c in A.level_sizes(t) if h % 8 == 0 and w % 16 == 0 and h * w >= 1024] for t in A.ARCHS}
    assert {t for t, v in big.items() if v} == {"rect", "wide3", "deep", "c192", "c128a"}
    assert {t for t, v in big.items() if any(c % 64 == 0 for _, _, c in v)} == {"rect", "wide3", "c192", "c128a"}
    # ... (deep's is 32 wide: its Winograd launches are the 64-channel convs of the block that up-samples into that level)
    assert big["deep"] == [(32, 32, 32)] and A.level_sizes("deep")[1] == (16, 16, 64) and A.PATHS["deep"]["wino"]
    assert {t for t in A.ARCHS if A.PATHS[t]["wino"]} == {t for t, v in big.items() if v}
    # a smaller level on whole 8 x 16 tiles whose width is whole 32-channel blocks: the split Winograd kernel
    small = {t: [(h, w, c) for h, w, c in A.level_sizes(t) if h % 8 == 0 and w % 16 == 0 and h * w < 1024 and c % 32 == 0] for t in A.ARCHS}
    assert {t for t, v in small.items() if v} == {"wide3", "deep", "nrb3", "c128a"} == {t for t in A.ARCHS if A.PATHS[t]["split"]}
    assert small["nrb3"] == [(16, 32, 128), (8, 16, 64)]
    # rows with neither
    assert {t for t in A.ARCHS if not big[t] and not small[t]} == {"one", "ragged", "narrow", "ch24", "attn_rag"}
    assert A.level_sizes("rect")[1] == (16, 24, 128) and A.level_sizes("ragged") == [(12, 20, 64), (6, 10, 64), (3, 5, 128)]
    assert A.level_sizes("attn_rag") == [(20, 20, 64), (10, 10, 128)]
    # parameter counts, the skip stack (num_res_blocks + 1 decoder blocks per level), the channel counts of the plain row
    assert len(A.orc.param_shapes(A.cfg_of("deep"))) == 432
    spec = A.orc.build_spec(A.cfg_of("deep"))
    assert len(spec.enc) + len(spec.dec) == 35 and sum(b.key.startswith("dec.32x32_block") for b in spec.dec) == 3
    assert sum(b.key.startswith("dec.16x32_block") or b.key.startswith("dec.16x16_block") for b in A.orc.build_spec(A.cfg_of("nrb3")).dec) == 4
    shapes = dict(A.orc.param_shapes(A.cfg_of("ch24")))
    assert shapes["enc.16x16_conv.weight"] == (24, 1, 3, 3) and shapes["out_conv.weight"] == (3, 24, 3, 3)
    assert dict(A.orc.param_shapes(A.cfg_of("c128a")))["dec.32x32_block0.skip.weight"] == (128, 256, 1, 1)
    assert dict(A.orc.param_shapes(A.cfg_of("rect")))["enc.16x16_block0.skip.weight"] == (128, 64, 1, 1)
    assert set(A.PATHS) == set(A.ARCHS) and all(t in A.ARCHS for rows, _ in list(A.SWITCHED.values()) + list(A.SWITCHED_TRAINING.values()) for t in rows)
