"""Host-side checker of the fused GroupNorm statistics chain, in fp64 on the CPU (plain torch; nothing here touches the GPU).

A producing conv writes, per sample, pixel tile and block of rc consecutive channels, a record (sum, M2): the sum of the block's
values inside the tile and their squared deviations from the record's OWN mean (csrc/common.hpp, SumTiles; conv_tile.hpp,
conv_epilogue).  The consumers (conv_tile.hpp stage_coef_rows, norm_emb_attn.hip gn_coef_from_sums_kernel) merge the records of a
GroupNorm group in fp64 (Chan et al.), with a tile's element count recomputed from the geometry.

A tiling is the five SumTiles fields (tiles, tiles_x, ph, pw, rc); a table is [B, tiles, C / rc, 2].  The 8-wave kernel's
records are per 8 x 32 SUB-tile of its 16 x 32 tile and its launcher reports exactly that geometry, so it is no special case here.
"""
import math
from collections import namedtuple

import torch

U = 2.0 ** -24                        # unit round-off of fp32 (round to nearest)
N_MAX = 4096                          # largest record the error analysis below is written for (the largest a kernel writes: 2048)

Records64 = namedtuple("Records64", "count sum m2 sum_abs max_abs")     # count [tiles]; the others [B, tiles, C / rc]


def tile_grid(tiling, H, W):
    tiles, tiles_x, ph, pw, rc = (int(v) for v in tiling)
    assert ph > 0 and pw > 0 and rc in (2, 4), tiling
    tiles_y = -(-H // ph)
    assert tiles_x == -(-W // pw) and tiles == tiles_x * tiles_y, f"tiling {tuple(tiling)} does not cover a {H} x {W} image"
    return tiles, tiles_x, tiles_y, ph, pw, rc


def tile_records64(y, tiling):
    """The exact records of y [B, C, H, W] (any float type, taken as it is) for the geometry `tiling`: ragged last tiles in both
    directions hold the live pixels only.  -> Records64 (with sum |v| and max |v| per record, which the error bounds need)."""
    y = y.detach().cpu().double()
    B, C, H, W = y.shape
    tiles, tiles_x, tiles_y, ph, pw, rc = tile_grid(tiling, H, W)
    assert C % rc == 0, (C, rc)
    nrec = C // rc
    count = torch.zeros(tiles, dtype=torch.int64)
    out = [torch.zeros(B, tiles, nrec, dtype=torch.float64) for _ in range(4)]
    for ty in range(tiles_y):
        for tx in range(tiles_x):
            t = ty * tiles_x + tx
            v = y[:, :, ty * ph:min(H, (ty + 1) * ph), tx * pw:min(W, (tx + 1) * pw)].reshape(B, nrec, -1)
            count[t] = v.shape[-1]
            s = v.sum(-1)
            out[0][:, t] = s
            out[1][:, t] = ((v - (s / v.shape[-1])[..., None]) ** 2).sum(-1)
            out[2][:, t] = v.abs().sum(-1)
            out[3][:, t] = v.abs().amax(-1)
    return Records64(count, *out)


def synthetic_records(y, tiling):
    """tile_records64 rounded to fp32, in the table layout [B, tiles, C / rc, 2]: drives a consumer without a producer."""
    r = tile_records64(y, tiling)
    return torch.stack([r.sum, r.m2], -1).float().contiguous()


def _source(records, tiling, H, W, C):
    records = records.detach().cpu().double()
    tiles, tiles_x, tiles_y, ph, pw, rc = tile_grid(tiling, H, W)
    assert tuple(records.shape[1:]) == (tiles, C // rc, 2) and C % rc == 0, (tuple(records.shape), tiling, C)
    hs = torch.tensor([min(ph, H - ty * ph) for ty in range(tiles_y)], dtype=torch.float64)
    ws = torch.tensor([min(pw, W - tx * pw) for tx in range(tiles_x)], dtype=torch.float64)
    n = (rc * hs[:, None] * ws[None, :]).reshape(-1)          # elements of a record of tile t (sum_tile_count)
    return records, n, rc


def merge64(records, tiling, H, W, groups, Ca, Cb=0, records_b=None, tiling_b=None, eps=1e-5):
    """The merge the consumers perform, in fp64: group mean and rstd [B, groups] of cat(a, b) [B, Ca + Cb, H, W] from the records
    of a (and of b, with a tiling and a record width of its own).  A group is a whole number of records of each table it touches
    and may straddle the concat boundary.  M2 = sum_t M2_t + sum_t n_t (mean_t - mean)^2: the consumers' formula
    sum_t M2_t + sum_t s_t^2 / n_t - S^2 / N in the form that does not cancel."""
    C = Ca + Cb
    assert C % groups == 0
    cpg = C // groups
    srcs = [_source(records, tiling, H, W, Ca) + (0, Ca)]
    if Cb:
        srcs.append(_source(records_b, tiling_b, H, W, Cb) + (Ca, Cb))
    B = srcs[0][0].shape[0]
    mean, rstd = torch.zeros(B, groups, dtype=torch.float64), torch.zeros(B, groups, dtype=torch.float64)
    N = float(cpg * H * W)
    for g in range(groups):
        c0 = g * cpg
        parts = []                                           # (sum, m2, n) of every record of the group, each [B, k]
        for rec, n, rc, base, Cs in srcs:
            lo, hi = max(c0, base), min(c0 + cpg, base + Cs)
            if lo >= hi:
                continue
            assert (lo - base) % rc == 0 and (hi - base) % rc == 0, "a group must be whole records of each source"
            r = rec[:, :, (lo - base) // rc:(hi - base) // rc]                 # [B, tiles, k, 2]
            parts.append((r[..., 0].reshape(B, -1), r[..., 1].reshape(B, -1), n[:, None].expand(-1, r.shape[2]).reshape(-1)))
        s, m2, n = (torch.cat([p[i] for p in parts], -1) for i in range(3))
        assert float(n.sum()) == N
        m = s.sum(-1) / N
        M2 = m2.sum(-1) + (n * (s / n - m[:, None]) ** 2).sum(-1)
        mean[:, g], rstd[:, g] = m, 1.0 / torch.sqrt(M2 / N + eps)
    return mean, rstd


def group_stats64(x, groups, eps=1e-5):
    """mean, rstd [B, groups] of x [B, C, H, W] in fp64, straight from the tensor."""
    xr = x.detach().cpu().double().reshape(x.shape[0], groups, -1)
    return xr.mean(-1), 1.0 / torch.sqrt(xr.var(-1, unbiased=False) + eps)


# Error bounds of a record against the fp64 record of the SAME fp32 values (the kernel's own output, read back).  u = 2^-24, n the
# record's element count, first order in u (the (n u)^2 terms are below 0.1 % of the bounds at n <= N_MAX).
#
# sum.  A record's sum is a tree of n - 1 fp32 additions in some order (serial over a lane's registers, butterfly over lanes, serial
# over waves).  Every addition rounds its result by a relative u, and a value passes through at most n - 1 of them, so whatever the
# order  |sum - sum64| <= (n - 1) u sum|v| <= n u sum|v|.
#
# M2.  The kernels take two passes over the accumulator registers: the sum above, the mean a = fl(sum / n), then fl(sum (v - a)^2).
#   * a is off the true mean m by at most  (n - 1) u sum|v| / n + u |m| <= n u max|v| =: delta.
#   * For ANY a, sum (v - a)^2 = M2_64 + n (a - m)^2 exactly: a wrong centre adds at most n delta^2.
#   * Evaluating it in fp32: d = fl(v - a) (relative u), fl(d * d + acc) (u for the fused multiply-add) and the n - 1 further
#     additions of the tree, all on non-negative terms: relative (n + 2) u <= 4 n u on the total.
#   Together  |M2 - M2_64| <= 4 n u M2_64 + n delta^2.
#   A tile written by several waves merges per-wave records (n_w, s_w, M2_w about a_w = fl(s_w / n_w)) as
#   sum_w [M2_w + n_w (a_w - a)^2] (conv_stats_combine).  That is sum (v - a)^2 - 2 sum_w n_w (a_w - a)(m_w - a_w): the same quantity
#   up to a cross term <= 2 delta_w sqrt(n B2) (Cauchy-Schwarz), B2 = sum_w n_w (a_w - a)^2 <= M2_64 the between-wave part of M2 and
#   delta_w = n_w u max|v| the error of a wave's mean.  The first term needs (n + 2) u M2_64 and leaves (3 n - 2) u M2_64 unused; with
#   the tile split over 8 half-waves (n_w = n / 8) the cross term fits there when (n / 4) max|v| sqrt(n B2) <= (3 n - 2) M2_64.  For
#   values without structure across the half-waves, B2 ~ 7 M2_64 / n and M2_64 = n std^2, that reads max|v| <= 4.5 sqrt(n) std, even
#   if every wave's mean were off by its worst case in the worst direction.  The tests' inputs (|mean| / std ~ 30; 36 std at the
#   smallest record, n = 64, 144 std at n = 1024) stay at or below it, which is why their means are not larger still.
def record_bounds(ref):
    n = ref.count.double()[None, :, None]
    assert int(ref.count.max()) <= N_MAX
    delta = n * U * ref.max_abs
    return n * U * ref.sum_abs, 4 * n * U * ref.m2 + n * delta ** 2


def record_errors(records, y_dev, tiling):
    """-> (err / bound of every sum, of every M2), each [B, tiles, C / rc]; a NaN record counts as infinitely wrong."""
    ref = tile_records64(y_dev, tiling)
    rec = records.detach().cpu().double()
    assert tuple(rec.shape) == tuple(ref.sum.shape) + (2,), (tuple(rec.shape), tuple(ref.sum.shape))
    bs, bm = record_bounds(ref)
    tiny = torch.finfo(torch.float64).tiny
    rs = (rec[..., 0] - ref.sum).abs() / bs.clamp_min(tiny)
    rm = (rec[..., 1] - ref.m2).abs() / bm.clamp_min(tiny)
    return torch.nan_to_num(rs, nan=math.inf), torch.nan_to_num(rm, nan=math.inf)


def check_records(records, y_dev, tiling, what=""):
    """Every record against the fp64 record of y_dev, the producing kernel's own fp32 output read back, at the bounds above.
    -> the largest err / bound (<= 1)."""
    rs, rm = record_errors(records, y_dev, tiling)
    worst_s, worst_m = float(rs.max()), float(rm.max())
    assert worst_s <= 1.0, f"{what}: {int((rs > 1).sum())} of {rs.numel()} record sums out of bound, worst err / bound {worst_s:.3e} at {_where(rs)}"
    assert worst_m <= 1.0, f"{what}: {int((rm > 1).sum())} of {rm.numel()} record M2s out of bound, worst err / bound {worst_m:.3e} at {_where(rm)}"
    return max(worst_s, worst_m)


def _where(r):
    i = int(r.argmax())
    return "(sample, tile, record) = " + str(tuple(int(v) for v in torch.unravel_index(torch.tensor(i), r.shape)))


def check_groups(got_mean, got_rstd, ref_mean, ref_rstd, rtol=1e-4, atol=1e-5, what=""):
    """Group statistics against the fp64 ones at the bar of test_gn_coef_golden (rtol 1e-4, atol 1e-5).  -> largest err / bound."""
    worst = 0.0
    for name, got, ref in (("mean", got_mean, ref_mean), ("rstd", got_rstd, ref_rstd)):
        got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
        assert got.shape == ref.shape, (what, name, got.shape, ref.shape)
        ratio = (got - ref).abs() / (atol + rtol * ref.abs())
        ratio = torch.nan_to_num(ratio, nan=math.inf)
        assert float(ratio.max()) <= 1.0, f"{what}: group {name} off, worst err / bound {float(ratio.max()):.3e}"
        worst = max(worst, float(ratio.max()))
    return worst
