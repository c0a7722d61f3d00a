"""GPU: the attention backward (csrc/bwd_kernels.hip launch_attention_bwd) on every launch branch -- the LDS-staged kernels with
and without the block remap, and the direct-from-global kernels with one, two and four waves per tile, on ragged and whole
tiles and for callers whose buffers are not 16-byte aligned (tests/_attn_bwd.py) -- against fp64 autograd through the oracle at
the project's bar (rtol 1e-4, atol 1e-5 max|ref| per tensor), the forward output `a` of op_attention included.  Per case: dqkv
is handed in full of NaN and comes back finite, the profiler shows the row `_attn_bwd.branch` predicts and no other
attention_bwd* row, a second call gives the same bits, and sample B - 1 of the batched call equals the B = 1 call bit for bit.

Worst err / bar against fp64 per case (<= 1 passes), "a | dqkv", as these tests print it on an MI355X ("-": the kind does not
exist for the case: the spikes need token 5, spike_kw a second wave).  "+4": that pointer one float past a 16-byte boundary.

    case                      branch     plain            spike            spike_kw         da50             x6
    T1-2x1x1x1                direct<1>  0.0000 | 0.0132  -                -                0.0000 | 0.0169  0.0000 | 0.3786
    T31-1x2x1x31              direct<1>  0.0285 | 0.0127  0.0101 | 0.0532  -                0.0285 | 0.0062  0.1252 | 0.2888
    T32-2x1x4x8               direct<1>  0.0213 | 0.0144  0.0223 | 0.0430  -                0.0213 | 0.0137  0.1151 | 0.1417
    T33-1x1x3x11              direct<1>  0.0162 | 0.0212  0.0193 | 0.0420  -                0.0162 | 0.0116  0.1627 | 0.2378
    T63-1x2x7x9               direct<1>  0.0305 | 0.0157  0.0108 | 0.0475  -                0.0305 | 0.0165  0.1767 | 0.2633
    T65-1x2x5x13              direct<2>  0.0296 | 0.0230  0.0153 | 0.0331  0.0133 | 0.0401  0.0296 | 0.0138  0.4487 | 0.3849
    T96-1x2x8x12              direct<2>  0.0246 | 0.0201  0.0109 | 0.0423  0.0099 | 0.0650  0.0246 | 0.0131  0.3648 | 0.2046
    T100-2x2x10x10            direct<2>  0.0276 | 0.0199  0.0138 | 0.0368  0.0133 | 0.0480  0.0276 | 0.0269  0.3517 | 0.4529
    T127-1x1x1x127            direct<2>  0.0190 | 0.0397  0.0109 | 0.0534  0.0166 | 0.0289  0.0190 | 0.0346  0.2924 | 0.2931
    T129-1x1x3x43             direct<4>  0.0242 | 0.0362  0.0105 | 0.0134  0.0144 | 0.0842  0.0242 | 0.0116  0.4055 | 0.2227
    T144-2x2x12x12            direct<4>  0.0269 | 0.0281  0.0105 | 0.0299  0.0101 | 0.0230  0.0269 | 0.0230  0.3562 | 0.1696
    T169-1x1x13x13            direct<4>  0.0255 | 0.0309  0.0119 | 0.0541  0.0149 | 0.0442  0.0255 | 0.0197  0.2920 | 0.3282
    T210-1x2x14x15            direct<4>  0.0264 | 0.0263  0.0149 | 0.0267  0.0114 | 0.0427  0.0264 | 0.0091  0.3086 | 0.1549
    T240-1x2x12x20            direct<4>  0.0389 | 0.0493  0.0135 | 0.0304  0.0156 | 0.0388  0.0389 | 0.0195  0.6860 | 0.3190
    T400-1x1x20x20            direct<4>  0.0421 | 0.0412  0.0113 | 0.0252  0.0106 | 0.0338  0.0421 | 0.0120  0.5666 | 0.4502
    T529-1x1x23x23            direct<4>  0.0275 | 0.0370  0.0132 | 0.0171  0.0168 | 0.0311  0.0275 | 0.0108  0.9411 | 0.4534
    T128-2x2x8x16-qkv+4       direct<4>  0.0324 | 0.0239  0.0179 | 0.0538  0.0154 | 0.0951  0.0324 | 0.0148  0.2645 | 0.3556
    T256-4x2x16x16-qkv+4      direct<4>  0.0293 | 0.0284  0.0111 | 0.0299  0.0133 | 0.0404  0.0293 | 0.0329  0.6902 | 0.9844
    T128-2x2x8x16-da+4        direct<4>  0.0324 | 0.0239  0.0179 | 0.0538  0.0154 | 0.0951  0.0324 | 0.0148  0.2645 | 0.3556
    T256-4x2x16x16-da+4       direct<4>  0.0293 | 0.0284  0.0111 | 0.0299  0.0133 | 0.0404  0.0293 | 0.0329  0.6902 | 0.9844
    T128-2x2x8x16             lds        0.0324 | 0.0235  0.0179 | 0.0538  0.0154 | 0.0950  0.0324 | 0.0192  0.2645 | 0.3562
    T384-1x1x16x24            lds        0.0283 | 0.0310  0.0095 | 0.0211  0.0099 | 0.0635  0.0283 | 0.0316  0.4762 | 0.2152
    T256-4x2x16x16            lds        0.0293 | 0.0292  0.0111 | 0.0235  0.0133 | 0.0399  0.0293 | 0.0271  0.6902 | 0.9847
    T384-8x1x16x24            lds        0.0381 | 0.0193  0.0107 | 0.0312  0.0124 | 0.0767  0.0381 | 0.0289  0.6306 | 0.3964
    T512-8x1x16x32            lds        0.0219 | 0.0403  0.0175 | 0.0379  0.0172 | 0.0665  0.0219 | 0.0302  0.8063 | 0.3396

The misaligned rows against the aligned (LDS) call on the same values: at most 0.078 of the bar.  x6 is where fp32 itself comes
close to the bar (PyTorch's fp32 autograd on the CPU: up to 0.86 on `a`, 0.63 on dqkv, tests/test_attn_bwd_cpu.py); before the
four-wave kernels took the forward's score units (csrc/bwd_kernels.hip AttnBwdUnits) their x6 column read 0.55 to 2.04 on dqkv.
"""
import pytest
import torch

from tests import _attn_bwd as AB

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    import mcedm_amd  # noqa: F401
    from mcedm_amd import lib as L
    assert torch.cuda.is_available()
    L.load()
    return L


def dev(t, off=False):
    """t on the device; off: as a view one float past a 16-byte boundary of a buffer that holds it whole."""
    t = t.detach().contiguous()
    if not off:
        d = t.cuda()
        assert d.data_ptr() % 16 == 0
        return d
    buf = torch.zeros(t.numel() + 4, device="cuda")
    d = buf[1:1 + t.numel()].view(t.shape)
    d.copy_(t)
    assert d.data_ptr() % 16 == 4 and d.is_contiguous()
    return d


def backward(L, pq, a, da, heads):
    """op_attention_bwd into a NaN-filled dqkv with the profiler on -> (dqkv, {attention_bwd* row: launches})."""
    out = torch.full(pq.shape, float("nan"), device="cuda")
    torch.cuda.synchronize()
    L.prof_enable(True)
    try:
        got = L.op_attention_bwd(pq, a, da, heads, out=out)
        torch.cuda.synchronize()
        rows = {r["name"]: int(r["launches"]) for r in L.prof_report() if r["name"].startswith("attention_bwd")}
    finally:
        L.prof_enable(False)
    assert got is out
    return out, rows


def run(L, case, kind, misalign, sample=None, a=None):
    """-> (a, dqkv, rows) in the kernels' packed layout; sample: that sample alone, as a batch of one."""
    qkv, da = AB.inputs(case, kind)
    if sample is not None:
        qkv, da = qkv[sample:sample + 1], da[sample:sample + 1]
    pq, dda = dev(AB.packed_qkv(qkv, case.heads), misalign == "qkv"), dev(da, misalign == "da")
    if a is None:
        a = L.op_attention(pq, case.heads)
    return (a,) + backward(L, pq, a, dda, case.heads)


@pytest.mark.parametrize("case,kind", AB.ALL, ids=AB.IDS)
def test_attention_backward_branch_vs_fp64(lib, case, kind):
    a64, g64 = AB.reference(case, kind)
    a, dqkv, rows = run(lib, case, kind, case.misalign)
    assert rows == {AB.row(case): 1}, (rows, AB.row(case))
    assert bool(torch.isfinite(dqkv).all()), int((~torch.isfinite(dqkv)).sum())
    got = AB.unpacked_qkv(dqkv.cpu(), case.heads)
    ra, rg = AB.bar_ratio(a, a64), AB.bar_ratio(got, g64)
    print(f"{case.id}-{kind}: err / bar vs fp64: a {ra:.4f}, dqkv {rg:.4f}")
    assert ra <= 1.0 and rg <= 1.0, (ra, rg)
    # a second call: the same bits
    _, again, _ = run(lib, case, kind, case.misalign, a=a)
    assert torch.equal(dqkv, again), float((dqkv - again).abs().max())
    # the last sample alone: the same bits (the kernels are chosen by T and alignment, never by the batch size, and the block remap
    # of the LDS kernels is a bijection of the grid)
    if case.B > 1:
        a1, alone, rows1 = run(lib, case, kind, case.misalign, sample=case.B - 1)
        assert rows1 == rows
        assert torch.equal(a1[0], a[-1]), float((a1[0] - a[-1]).abs().max())
        assert torch.equal(alone[0], dqkv[-1]), float((alone[0] - dqkv[-1]).abs().max())
    if case.misalign:
        # the same values from aligned buffers take the LDS kernels; the two agree at the bar
        _, lds, rows_al = run(lib, case, kind, None)
        assert rows_al == {"attention_bwd_lds": 1}, rows_al
        r = AB.bar_ratio(dqkv, lds.cpu())
        print(f"{case.id}-{kind}: err / bar vs the aligned call: dqkv {r:.4f}")
        assert r <= 1.0, r


def test_out_is_checked(lib):
    case = AB.CASES[2]
    qkv, da = AB.inputs(case, "plain")
    pq, dda = dev(AB.packed_qkv(qkv, case.heads)), dev(da)
    a = lib.op_attention(pq, case.heads)
    with pytest.raises(ValueError, match="shape"):
        lib.op_attention_bwd(pq, a, dda, case.heads, out=torch.empty(pq.numel(), device="cuda"))
    # without `out` the entry allocates the result itself, as before
    assert torch.equal(lib.op_attention_bwd(pq, a, dda, case.heads), backward(lib, pq, a, dda, case.heads)[0])
