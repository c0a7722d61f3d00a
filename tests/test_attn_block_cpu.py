"""CPU side of the fused attention block's kernel-level tests (tests/test_hip_attn_block.py): the reference's arithmetic in fp32
meets its fp64 evaluation within the project's bar on every case -- so the bar needs no widening for the kernel --, and every case
is in the regime it is there for.  A change to the fixtures that turned the cases back into uniform-softmax ones fails here."""
import torch

from oracle import mcedm_oracle as orc
from tests import _attn_block as AB


def key_slots(keys):
    """(key block, half-wave) of keys as attn_block64_kernel holds them: key = 32 kb + (r & 3) + 8 (r >> 2) + 4 (lane >> 5)."""
    return {(int(k) >> 5, (int(k) >> 2) & 1) for k in keys.flatten()}


def tail_one_pass_variance(P, y):
    """AB.tail in fp32 with the GroupNorm variance taken as E[x^2] - mean^2: the shortcut the kernel's two passes avoid."""
    x = y.reshape(y.shape[0], 16, -1)
    mean = x.sum(-1, keepdim=True) / 256
    var = (x * x).sum(-1, keepdim=True) / 256 - mean * mean
    xn = ((x - mean) / torch.sqrt(var + 1e-5)).reshape(y.shape)
    h = xn * P["norm2.weight"].reshape(1, -1, 1, 1) + P["norm2.bias"].reshape(1, -1, 1, 1)
    qkv = orc.conv2d(h, P["qkv.weight"], P["qkv.bias"])
    return orc.conv2d(orc.attention(qkv, 1), P["proj.weight"], P["proj.bias"]) + y


def test_fp32_reference_meets_fp64_and_every_case_is_in_its_regime():
    every_slot = {(0, 0), (0, 1), (1, 0), (1, 1)}
    for name, (qk, proj, diag, kind) in AB.CASES.items():
        P, y = AB.case(name)
        with torch.no_grad():
            z32 = AB.tail(P, y)
        z64, qkv = AB.tail64(P, y, want_qkv=True)
        w = AB.worst(z32, z64)
        r = AB.regime(P, y)
        print(f"{name}: fp32 reference / bar {w:.4f}  " + "  ".join(f"{k} {v:.4g}" for k, v in r.items()))
        assert w < 1.0, (name, w)
        q, k, _ = qkv.reshape(3, 64, 3, 64).unbind(2)
        p = torch.einsum("ncq,nck->nqk", q, k / 8).softmax(2)
        if proj == 8.0:
            assert r["share"] > 0.25, (name, r)
        if name.startswith("peak"):       # the maxima fall in either key block and either half-wave
            assert key_slots(p.argmax(2)) == every_slot, name
        if name == "plain":               # the baseline is what the network tests already exercise: uniform attention
            assert r["smax"] < 0.05 and r["ptop_median"] < 1.02 / 64, r
        if name == "peak20":
            assert r["smax"] > 4 and 0.05 < r["ptop_median"] < 0.3, r
        if name == "peak40":
            assert r["smax"] > 18 and 0.3 < r["ptop_median"] < 0.9, r
        if name == "peak80":
            assert r["ptop_median"] > 0.9, r
        if name == "peak120":             # exp overflows in fp32 unless the merged maximum is subtracted
            assert r["smax"] > 88, r
        if name == "diag":
            # k = q makes the scores a Gram matrix (symmetric).  That puts query t's own key on top with probability > 0.999 for
            # the longer q_t only -- a short q_t scores higher against a longer, aligned q_u than against itself --, which is a
            # quarter of the queries at least, in every key block and half-wave: for those a key / probability pairing error in
            # the P.V product is an O(1) error at a known key.
            s = torch.einsum("ncq,nck->nqk", q, k / 8)
            assert float((s - s.transpose(1, 2)).abs().max()) <= 1e-12 * r["smax"], "diag: scores are not a Gram matrix"
            own = p.diagonal(dim1=1, dim2=2) > 0.999
            assert float(own.float().mean()) > 0.25, float(own.float().mean())
            assert key_slots(torch.nonzero(own)[:, 1]) == every_slot
        g = y.double().reshape(3, 16, -1)
        if kind == "mean300":
            assert float((g.mean(-1).abs() / g.std(-1)).min()) > 500
        if kind == "tight":               # a one-pass variance in fp32 must be far outside the bar here (it is not on mean300)
            assert float((g.mean(-1).abs() / g.std(-1)).min()) > 500 and r["share"] > 0.2, r
            with torch.no_grad():
                assert AB.worst(tail_one_pass_variance(P, y), z64) > 10
        if kind == "groups160":
            assert float(g.mean(-1).min()) < -150 and float(g.mean(-1).max()) > 130
        if kind == "const":
            assert float(g.var(-1, unbiased=False)[:, 5].max()) == 0.0 and float(g.var(-1, unbiased=False)[:, 4].min()) > 0.5
