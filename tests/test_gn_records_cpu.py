"""tests/_gn_records.py, the fp64 checker of the fused GroupNorm records, checked itself (CPU only, seconds):
  * tile_records64 followed by merge64 is torch's fp64 mean / variance to 1e-12, over ragged tilings in both directions, pair and
    quad records, the 8-row sub-tiles of the 8-wave kernel, two sources with different tilings and record widths, a group across
    the concat boundary, and data whose mean is 40+ standard deviations;
  * check_records would fail a subtly wrong kernel: four corruptions of correct records are each rejected -- and the group-level
    check alone accepts records stored under the wrong (equal-sized) tile, which is why the per-record check exists."""
import pytest
import torch

from oracle import fixtures as fx
from tests import _gn_records as R


def big_mean(tag, B, C, H, W, mean=50.0):
    """|mean| / std >= 40 per group, a mean per channel and a slope down the rows (so that tile, record and group means all differ)."""
    ch = mean * (1 - 2 * (torch.arange(C) // 4 % 2)).float() + 0.2 * fx.randn(tag + "/ch", C)
    return fx.randn(tag, B, C, H, W) + ch[None, :, None, None] + 0.02 * torch.arange(H).float()[None, None, :, None]


GEOMETRIES = [
    # (C, H, W, (ph, pw, rc), groups)
    (64, 40, 24, (8, 32, 4), 16), (64, 40, 24, (16, 16, 2), 32), (128, 40, 24, (8, 8, 4), 32), (8, 20, 12, (8, 8, 2), 2),
    (16, 80, 72, (4, 8, 4), 4), (16, 12, 10, (8, 16, 2), 8), (64, 16, 32, (8, 16, 4), 4), (8, 40, 40, (8, 32, 4), 2),
]


def tiling_of(H, W, ph, pw, rc):
    tx = -(-W // pw)
    return (tx * -(-H // ph), tx, ph, pw, rc)


@pytest.mark.parametrize("geom", GEOMETRIES)
def test_merge_of_exact_records_is_the_fp64_group_statistic(geom):
    C, H, W, (ph, pw, rc), groups = geom
    x = big_mean("gnrec/cpu/" + "_".join(map(str, (C, H, W, ph, pw, rc))), 2, C, H, W).double()
    tiling = tiling_of(H, W, ph, pw, rc)
    r = R.tile_records64(x, tiling)
    assert int(r.count.sum()) == rc * H * W and int(r.count.max()) == rc * min(ph, H) * min(pw, W)
    mean, rstd = R.merge64(torch.stack([r.sum, r.m2], -1), tiling, H, W, groups, C)
    xr = x.reshape(2, groups, -1)
    ref_mean, ref_var = xr.mean(-1), xr.var(-1, unbiased=False)
    if C // groups <= 4:          # (wider groups mix channels of both signs)
        assert float((ref_mean.abs() / ref_var.sqrt()).min()) >= 40
    torch.testing.assert_close(mean, ref_mean, rtol=1e-12, atol=0)
    torch.testing.assert_close(rstd, 1 / torch.sqrt(ref_var + 1e-5), rtol=1e-12, atol=0)
    g_mean, g_rstd = R.group_stats64(x, groups)
    torch.testing.assert_close(g_mean, ref_mean, rtol=1e-14, atol=0)
    torch.testing.assert_close(g_rstd, 1 / torch.sqrt(ref_var + 1e-5), rtol=1e-14, atol=0)


@pytest.mark.parametrize("Ca,Cb,ta,tb,groups", [
    (64, 192, (8, 8, 2), (8, 16, 4), 32),          # pairs | quads, different tilings, 8-channel groups
    (132, 124, (8, 32, 4), (16, 16, 4), 32),       # the group of channels 128-135 straddles the boundary
    (4, 4, (4, 8, 2), (8, 8, 4), 1),               # one group over both sources
])
def test_merge_of_two_sources(Ca, Cb, ta, tb, groups):
    H, W = 20, 24
    a, b = big_mean(f"gnrec/cpu/cat{Ca}/a", 3, Ca, H, W).double(), big_mean(f"gnrec/cpu/cat{Ca}/b", 3, Cb, H, W, mean=-35.0).double()
    tla, tlb = tiling_of(H, W, *ta), tiling_of(H, W, *tb)
    ra, rb = R.tile_records64(a, tla), R.tile_records64(b, tlb)
    mean, rstd = R.merge64(torch.stack([ra.sum, ra.m2], -1), tla, H, W, groups, Ca, Cb, torch.stack([rb.sum, rb.m2], -1), tlb)
    ref_mean, ref_rstd = R.group_stats64(torch.cat([a, b], 1), groups)
    torch.testing.assert_close(mean, ref_mean, rtol=1e-12, atol=1e-13)
    torch.testing.assert_close(rstd, ref_rstd, rtol=1e-12, atol=0)


def test_the_8_wave_geometry_is_rows_of_8():
    """The 8-wave kernel's 16 x 32 tile stores two 8 x 32 records; 40 rows leave the last tile one live sub-tile: five tile rows."""
    tiling = tiling_of(40, 24, 8, 32, 4)
    assert tiling == (5, 1, 8, 32, 4)
    r = R.tile_records64(torch.ones(1, 4, 40, 24), tiling)
    assert r.count.tolist() == [4 * 8 * 24] * 5 and torch.equal(r.sum, torch.full((1, 5, 1), 768.0, dtype=torch.float64))
    assert float(r.m2.abs().max()) == 0.0
    with pytest.raises(AssertionError, match="does not cover"):
        R.tile_records64(torch.ones(1, 4, 40, 24), (4, 1, 16, 32, 4))


@pytest.fixture(scope="module")
def ragged():
    """A ragged, large-mean fp32 tensor, as a kernel would have stored it: 20 x 12 in 8 x 8 tiles = 3 x 2 tiles of 8 x 8, 8 x 4
    (twice), 4 x 8 and 4 x 4 pixels."""
    y = big_mean("gnrec/cpu/ragged", 2, 8, 20, 12, mean=30.0)
    return y, {rc: tiling_of(20, 12, 8, 8, rc) for rc in (2, 4)}


def test_correct_records_pass(ragged):
    y, tilings = ragged
    for rc, tiling in tilings.items():
        worst = R.check_records(R.synthetic_records(y, tiling), y, tiling, what=f"rc {rc}")
        assert worst <= 1.0
        ref = R.tile_records64(y, tiling)
        assert ref.count.tolist() == [rc * n for n in (64, 32, 64, 32, 32, 16)]
        # fp32 records merge to the group statistics of the tensor at the bar of the GPU tests
        mean, rstd = R.merge64(R.synthetic_records(y, tiling), tiling, 20, 12, 2, 8)
        R.check_groups(mean, rstd, *R.group_stats64(y, 2), what=f"rc {rc}")
    nan = R.synthetic_records(y, tilings[4])
    nan[1, 3, 0, 1] = float("nan")
    with pytest.raises(AssertionError, match="M2s out of bound"):
        R.check_records(nan, y, tilings[4])


def test_check_records_rejects_four_subtly_wrong_kernels(ragged):
    y, tilings = ragged
    t4, t2 = tilings[4], tilings[2]
    good = R.synthetic_records(y, t4)
    ref_mean, ref_rstd = R.group_stats64(y, 2)

    # 1. two tiles of different element count stored under each other's index
    swapped = good.clone()
    swapped[:, [0, 1]] = good[:, [1, 0]]
    with pytest.raises(AssertionError, match="out of bound"):
        R.check_records(swapped, y, t4)

    # 2. M2 about the GROUP mean (here a group is one record's channels over the whole image) instead of the tile's own
    ref = R.tile_records64(y, t4)
    n = ref.count.double()[None, :, None]
    gmean = ref_mean[:, None, :]                                     # [B, 1, groups = records]
    about_group = good.clone()
    about_group[..., 1] = (ref.m2 + n * (ref.sum / n - gmean) ** 2).float()
    with pytest.raises(AssertionError, match="M2s out of bound"):
        R.check_records(about_group, y, t4)

    # 3. the last live row of the ragged bottom tiles left out (rows 16-18 of 16-19)
    short = good.clone()
    short[:, 4:] = R.synthetic_records(y[:, :, :19], (6, 2, 8, 8, 4))[:, 4:]
    with pytest.raises(AssertionError, match="sums out of bound"):
        R.check_records(short, y, t4)

    # 4. pair mode: the records of the two channel pairs of a quad exchanged
    pairs = R.synthetic_records(y, t2)
    crossed = pairs.clone()
    crossed[:, :, [0, 1]] = pairs[:, :, [1, 0]]
    with pytest.raises(AssertionError, match="out of bound"):
        R.check_records(crossed, y, t2)
    # (a group of the 2-group norm holds both pairs: the merged statistics cannot see this one at all)
    R.check_groups(*R.merge64(crossed, t2, 20, 12, 2, 8), ref_mean, ref_rstd)

    # Records under the wrong index of two EQUAL-sized tiles (0 and 2, both 8 x 8): the merged group statistics are unchanged, so
    # the group-level check accepts what the per-record check rejects.
    same = good.clone()
    same[:, [0, 2]] = good[:, [2, 0]]
    R.check_groups(*R.merge64(same, t4, 20, 12, 2, 8), ref_mean, ref_rstd, what="equal-sized swap")
    with pytest.raises(AssertionError, match="out of bound"):
        R.check_records(same, y, t4)
    # ... while the different-sized swap of 1. does reach the group statistics (the consumer recomputes the count from the index)
    with pytest.raises(AssertionError, match="group"):
        R.check_groups(*R.merge64(swapped, t4, 20, 12, 2, 8), ref_mean, ref_rstd)
