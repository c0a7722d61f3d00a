"""What the tests of the fused 8 x 8 x 64 attention block (csrc/attn_fused.hip, attn_block64_kernel) share: the cases, the fp64
reference z = proj(attention(qkv(group_norm(y)))) + y out of the oracle's own functions, the figures that say which regime a case
is in, and hip_block -- a UNetBlock composed from the kernel-level entries, with either form of the attention tail.

The fixture parameters alone give uniform attention (|s| <= 0.02, every probability 1/64 to 2 %) that is 6 % of z, so the cases
scale the q / k rows (and biases) of qkv and the proj weight until the softmax is peaked and the attention term is a third of z.
Nothing here needs a GPU to import; tests/test_attn_block_cpu.py holds the cases to the regimes they claim."""
import torch

from oracle import fixtures as fx
from oracle import mcedm_oracle as orc

RTOL, ATOL = 1e-4, 1e-5      # the project's bar (tests/test_hip_parity.py)
TAG = "t/ab"

# name -> (q/k scale, proj scale, k := q, input).  Inputs: "randn"; "mean300" = 300 + 0.5 randn; "groups160" = randn + 20 (g - 8)
# in 4-channel group g; "const" = randn with group 5 of every sample set to one value per sample; "tight" = 3 + 0.005 randn.
# mean300 and groups160 put large means into the GroupNorm but also into the residual, whose rtol then hides a GroupNorm error of
# a few per cent; "tight" has the same |mean| / std = 600 on a residual of 3 under an attention term of 1, so it does not.
CASES = {
    "plain": (1.0, 1.0, False, "randn"),
    "peak20": (20.0, 8.0, False, "randn"),
    "peak40": (40.0, 8.0, False, "randn"),
    "peak80": (80.0, 8.0, False, "randn"),
    "peak120": (120.0, 8.0, False, "randn"),
    "diag": (60.0, 8.0, True, "randn"),
    "mean300": (6.0, 1.0, False, "mean300"),
    "groups160": (6.0, 1.0, False, "groups160"),
    "constgroup": (1.0, 1.0, False, "const"),
    "tight": (20.0, 24.0, False, "tight"),
}


def dev(t):
    return t.contiguous().cuda()


def params(qk=1.0, proj=1.0, diag=False):
    """norm2 / qkv / proj parameters of one block in the reference's layout (qkv rows 3 c + {q, k, v}, adm_blocks.py:175)."""
    P = {"norm2.weight": fx.param(TAG, "norm2.weight", (64,)), "norm2.bias": fx.param(TAG, "norm2.bias", (64,)),
         "qkv.weight": fx.param(TAG, "qkv.weight", (192, 64, 1, 1)).clone(), "qkv.bias": fx.param(TAG, "qkv.bias", (192,)).clone(),
         "proj.weight": fx.param(TAG, "proj.weight", (64, 64, 1, 1)) * proj, "proj.bias": fx.param(TAG, "proj.bias", (64,))}
    w, b = P["qkv.weight"].reshape(64, 3, 64), P["qkv.bias"].reshape(64, 3)      # views
    if diag:                       # k = q: the scores are a Gram matrix
        w[:, 1], b[:, 1] = w[:, 0], b[:, 0]
    w[:, :2] *= qk
    b[:, :2] *= qk
    return P


def inputs(kind, B=3, tag="y"):
    y = fx.randn(f"{TAG}/{tag}", B, 64, 8, 8)
    if kind == "mean300":
        return 300.0 + 0.5 * y
    if kind == "tight":
        return 3.0 + 0.005 * y
    if kind == "groups160":
        return y + ((torch.arange(16).float() - 8).repeat_interleave(4) * 20).reshape(1, 64, 1, 1)
    if kind == "const":
        y = y.clone()
        y[:, 20:24] = (0.7 + 0.3 * torch.arange(B).float()).reshape(B, 1, 1, 1)
        return y
    assert kind == "randn", kind
    return y


def case(name, B=3, tag="y"):
    qk, proj, diag, kind = CASES[name]
    return params(qk, proj, diag), inputs(kind, B, tag)


def tail(P, y, want_qkv=False):
    """adm_blocks.py:174-180 with the oracle's functions, in the dtype of its arguments."""
    qkv = orc.conv2d(orc.group_norm(y, P["norm2.weight"], P["norm2.bias"]), P["qkv.weight"], P["qkv.bias"])
    z = orc.conv2d(orc.attention(qkv, 1), P["proj.weight"], P["proj.bias"]) + y
    return (z, qkv) if want_qkv else z


def tail64(P, y, want_qkv=False):
    with torch.no_grad():
        return tail({k: v.double() for k, v in P.items()}, y.double(), want_qkv)


def regime(P, y):
    """fp64 figures of a case: largest |score|, median over the queries of the largest probability, the attention term's share of z."""
    z, qkv = tail64(P, y, want_qkv=True)
    q, k, _ = qkv.reshape(y.shape[0], 64, 3, 64).unbind(2)
    s = torch.einsum("ncq,nck->nqk", q, k / 8)
    p = s.softmax(2)
    return {"smax": float(s.abs().max()), "ptop_median": float(p.max(2).values.median()),
            "share": float((z - y.double()).abs().mean() / z.abs().mean())}


def worst(got, ref, rtol=RTOL, atol=ATOL):
    """Largest error in units of the bar atol + rtol |ref| (<= 1 passes `close`)."""
    got, ref = torch.as_tensor(got).detach().cpu().double(), torch.as_tensor(ref).detach().cpu().double()
    assert got.shape == ref.shape, (tuple(got.shape), tuple(ref.shape))
    return float(((got - ref).abs() / (atol + rtol * ref.abs())).max())


def group_stats64(z):
    """fp64 mean and rstd (eps 1e-5) of every 4-channel group of z [B, 64, 8, 8] -> two [B, 16] tensors."""
    g = z.double().reshape(z.shape[0], 16, -1)
    return g.mean(-1), 1 / (g.var(-1, unbiased=False) + 1e-5).sqrt()


def pack(L, P):
    """The device-side arguments of op_attn_block after y."""
    wq, bq = L.op_pack_conv(dev(P["qkv.weight"]), dev(P["qkv.bias"]), qkv_heads=1)
    wp, bp = L.op_pack_conv(dev(P["proj.weight"]), dev(P["proj.bias"]))
    return dev(P["norm2.weight"]), dev(P["norm2.bias"]), wq, bq, wp, bp


def three_launches(L, y, gamma, beta, wq, bq, wp, bp):
    """The same tail out of op_gn_coef, the 1x1 qkv conv, op_attention and the 1x1 proj conv with the residual."""
    qkv = L.op_conv(y, None, wq, bq, 192, 1, coef=L.op_gn_coef(y, None, gamma, beta))
    return L.op_conv(L.op_attention(qkv, 1), None, wp, bp, 64, 1, res=y)


def hip_block(L, P, spec, x, emb, fused_attn=False):
    """adm_blocks.py:159-181 composed from the kernel-level entry points (mirrors csrc/plan.hip run_block).  fused_attn: the attention
    tail is one op_attn_block call (64 channels at 8 x 8 only) instead of op_gn_coef, qkv conv, op_attention and proj conv."""
    k = spec.key
    g = lambda n: dev(P[f"{k}.{n}"])
    n_emb = emb.shape[0]
    film = dev(orc.linear(emb, P[f"{k}.affine.weight"], P[f"{k}.affine.bias"]))
    rs = L.RS_UP if spec.up else (L.RS_DOWN if spec.down else L.RS_NONE)
    xd = dev(x)
    c0 = L.op_gn_coef(xd, None, g("norm0.weight"), g("norm0.bias"))
    w0, b0 = L.op_pack_conv(g("conv0.weight"), g("conv0.bias"))
    h = L.op_conv(xd, None, w0, b0, spec.cout, 3, coef=c0, act=1, resample=rs)
    c1 = L.op_gn_coef(h, None, g("norm1.weight"), g("norm1.bias"), film=film, film_batch=int(n_emb > 1),
                      film_stride=2 * spec.cout)
    res, mode = xd, L.RS_NONE
    if spec.skip_kernel == 1:
        ws, bs = L.op_pack_conv(g("skip.weight"), g("skip.bias"))
        res = L.op_conv(xd, None, ws, bs, spec.cout, 1, resample=rs)
    elif spec.skip_kernel == 0:
        mode = rs
    w1, b1 = L.op_pack_conv(g("conv1.weight"), g("conv1.bias"))
    y = L.op_conv(h, None, w1, b1, spec.cout, 3, coef=c1, act=1, res=res, res_mode=mode)
    if not spec.attn:
        return y
    wq, bq = L.op_pack_conv(g("qkv.weight"), g("qkv.bias"), qkv_heads=spec.heads)
    wp, bp = L.op_pack_conv(g("proj.weight"), g("proj.bias"))
    if fused_attn:
        assert spec.heads == 1
        return L.op_attn_block(y, g("norm2.weight"), g("norm2.bias"), wq, bq, wp, bp)
    c2 = L.op_gn_coef(y, None, g("norm2.weight"), g("norm2.bias"))
    qkv = L.op_conv(y, None, wq, bq, 3 * spec.cout, 1, coef=c2)
    a = L.op_attention(qkv, spec.heads)
    return L.op_conv(a, None, wp, bp, spec.cout, 1, res=y)
