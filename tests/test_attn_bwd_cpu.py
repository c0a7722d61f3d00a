"""CPU checks of what the attention backward tests stand on (tests/_attn_bwd.py): the table reaches every launch branch and the
edges of each, the project's bar is fair to an fp32 kernel on every (case, kind), the plain inputs already tell a kernel that
masks one padding key too few from a correct one, and the fp64 reference agrees with the reference's own stored gradients."""
import pytest
import torch

from oracle import fixtures as fx
from tests import _attn_bwd as AB


def test_branch_restates_the_launcher():
    assert [AB.branch(T) for T in (1, 63, 64, 127, 128, 129, 255, 256, 257, 384, 400)] == [
        "direct<1>", "direct<1>", "direct<2>", "direct<2>", "lds", "direct<4>", "direct<4>", "lds", "direct<4>", "lds", "direct<4>"]
    assert [AB.branch(T, False) for T in (32, 64, 128, 256, 1024)] == ["direct<1>", "direct<2>", "direct<4>", "direct<4>", "direct<4>"]


def test_the_table_reaches_what_it_claims():
    by = {}
    for c in AB.CASES:
        by.setdefault(c.branch, []).append(c)
    assert set(by) == {"direct<1>", "direct<2>", "direct<4>", "lds"}
    T = {b: sorted({c.T for c in v}) for b, v in by.items()}
    assert T["direct<1>"] == [1, 31, 32, 33, 63]
    assert set(T["direct<2>"]) >= {65, 100, 127} and set(T["direct<4>"]) >= {129, 144, 240, 400, 529}
    assert T["lds"] == [128, 256, 384, 512]
    for b in ("direct<1>", "direct<2>", "direct<4>"):
        kw = AB.KW[b]
        assert all(AB.branch(t, False) == b for t in T[b])
        assert any(t % 32 for t in T[b]) and any(t % 32 == 0 for t in T[b]), (b, T[b])     # a ragged T and a whole-tile T
        last_wave = {((t - 1) // 32) % kw for t in T[b] if t % 32}                          # the wave that owns the ragged tile
        assert last_wave == set(range(kw)), (b, last_wave)
        assert any((t + 31) // 32 > kw for t in T[b]) or kw == 1                            # a wave that walks more than one tile
    assert any(t % 4 for t in T["direct<4>"]) and any(t % 2 for t in T["direct<4>"])
    # direct<4> on whole tiles exists only for misaligned callers: both pointers of the predicate, T = 128 and 256
    mis = {(c.misalign, c.T) for c in AB.CASES if c.misalign}
    assert mis == {(p, t) for p in ("qkv", "da") for t in (128, 256)} and all(c.branch == "direct<4>" for c in AB.CASES if c.misalign)
    for c in AB.CASES:                 # every misaligned row has its aligned twin to compare with
        assert c.misalign is None or c._replace(misalign=None) in AB.CASES
    # the LDS kernels with the block remap (xcd_group_map: B heads % 8 == 0) on 2, 3 and 4 workgroups per head, and without it
    assert {c.T // 128 for c in by["lds"] if c.B * c.heads % 8 == 0} == {2, 3, 4}
    assert {c.T // 128 for c in by["lds"] if c.B * c.heads % 8} == {1, 3}
    # more than one head, and a batch to take the last sample of, in every branch
    assert all(any(c.heads > 1 for c in v) and any(c.B > 1 for c in v) for v in by.values())
    # every kind on a ragged and on a whole-tile case of every branch it exists for (the LDS branch has whole tiles only)
    for b, v in by.items():
        for k in AB.KINDS:
            if k == "spike_kw" and AB.KW[b] == 1:
                continue
            shapes = {bool(c.T % 32) for c in v if k in AB.kinds(c)}
            assert shapes == ({False} if b == "lds" else {False, True}), (b, k, shapes)
    assert len(set(AB.IDS)) == len(AB.IDS)


def test_the_spikes_hold_the_row_maximum_where_they_claim():
    for c in AB.CASES:
        for k in ("spike", "spike_kw"):
            if k not in AB.kinds(c):
                continue
            key = c.T - 1 if k == "spike" else AB.spike_kw_key(c)
            assert key // 32 == ((c.T - 1) // 32 if k == "spike" else AB.KW[c.branch] - 1)      # the last tile / the last wave's first
            qkv, _ = AB.inputs(c, k)
            q, kk, _ = qkv.double().reshape(c.B * c.heads, 64, 3, c.T).unbind(2)
            s = torch.einsum("ncq,nck->nqk", q, kk / 8)
            assert bool((s[:, 5].argmax(-1) == key).all()) and float(s[:, 5, key].min()) > 20, (c.id, k)


FAIR = [(c, k) for c, k in AB.ALL if not c.misalign]      # the misaligned rows share the values of their aligned twins


@pytest.mark.parametrize("case,kind", FAIR, ids=[f"{c.id}-{k}" for c, k in FAIR])
def test_the_bar_is_fair_to_fp32(case, kind):
    """PyTorch's fp32 autograd through the oracle, the arithmetic the reference itself runs, sits within the bar of fp64 on every
    input the kernels are held to it on.  Worst measured, a or dqkv: plain and da50 0.052, the spikes 0.049, x6 0.86 (on `a` at
    T = 529; dqkv 0.63)."""
    a64, g64 = AB.reference(case, kind)
    a32, g32 = AB.autograd(*AB.inputs(case, kind), case.heads, torch.float32)
    ra, rg = AB.bar_ratio(a32, a64), AB.bar_ratio(g32, g64)
    print(f"{case.id}-{kind}: fp32 autograd vs fp64, err / bar: a {ra:.4f}, dqkv {rg:.4f}")
    assert bool(torch.isfinite(g64).all()) and ra <= 1.0 and rg <= 1.0, (ra, rg)


@pytest.mark.parametrize("case", [c for c in AB.CASES if c.T % 32], ids=lambda c: c.id)
def test_one_unmasked_padding_key_is_far_outside_the_bar(case):
    """A kernel that masked one key too few on the ragged tile would miss the bar by a factor of thousands on the plain inputs."""
    r = AB.bar_ratio(AB.one_key_unmasked(case), AB.reference(case, "plain")[1])
    print(f"{case.id}: one unmasked padding key, err / bar {r:.0f}")
    assert r > 100.0, r


@pytest.mark.parametrize("T", list(fx.ATTN_CASES))
def test_fp64_reference_agrees_with_the_stored_gradients(golden, T):
    B, hw = fx.ATTN_CASES[T]
    qkv = fx.randn(f"ops/attn{T}/qkv", B, 384, *hw)
    da = fx.randn(f"ops/attn{T}/da", B, 128, *hw)
    _, g = AB.autograd(qkv, da, 2)
    r = AB.bar_ratio(golden("ops.npz")[f"attn{T}_dqkv"], g)
    print(f"attn{T}_dqkv: the reference's fp32 vs fp64 autograd through the oracle, err / bar {r:.4f}")
    assert r <= 1.0, r
