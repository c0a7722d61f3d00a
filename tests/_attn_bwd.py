"""What the tests of the attention backward (csrc/bwd_kernels.hip launch_attention_bwd) share: the table of shapes, one or more per
launch branch, the input kinds, the fp64 reference (autograd through oracle.mcedm_oracle.attention on the fp32 inputs cast to
double) and `branch`, a restatement of the launcher's choice.  Nothing here needs a GPU to import; tests/test_attn_bwd_cpu.py
holds the table to the branches and edges it claims, and the inputs to the regime in which the project's bar is fair.

The launcher picks its kernels from the token count T = H W and the alignment of two pointers:

    lds        T % 128 == 0, qkv and da 16-byte aligned    attn_bwd_dq_lds_kernel, attn_bwd_dkv_lds_kernel (four waves, each walks
                                                           every 32-token chunk; block remap xcd_group_map where B heads % 8 == 0)
    direct<4>  otherwise, T >= 128                         attn_bwd_{stats,dq,dkv}_kernel<4>: the 32-token tiles w, w + KW, ... of
    direct<2>  64 <= T < 128                               the streamed axis on wave w, partial results merged through LDS in
    direct<1>  T < 64                                      wave order; a ragged last tile is loaded clamped and masked

With the knobs at their defaults lds and direct<4> form their scores in units of log 2 and direct<2>, direct<1> in natural units:
each as the forward kernel of the same T and knobs does (common.hpp attn_fwd_kernel, AttnBwdUnits; tests/_knobs.py): delta = sum_c da a carries the forward's probabilities, and the x6 inputs notice a backward whose
recomputed probabilities differ from them by one rounding of the scaled query.

Layouts: the oracle takes qkv [B, heads 3 64, H, W] in the reference's channel order (head, c, {q, k, v}); the kernels take the
packed order (head, {q, k, v}, c) that the qkv conv writes (packed_qkv / unpacked_qkv)."""
import collections
import functools

import torch

from oracle import fixtures as fx
from oracle import mcedm_oracle as orc
from tests._ddpm_arch import bar_ratio  # noqa: F401  (the project's bar: rtol 1e-4, atol 1e-5 max|ref| per tensor)

TAG = "t/attnbwd"
# waves per workgroup that share one tile of the kept axis (the LDS kernels: four tiles per workgroup, one per wave, no merge)
KW = {"direct<1>": 1, "direct<2>": 2, "direct<4>": 4, "lds": 4}


class Case(collections.namedtuple("Case", "B heads H W misalign")):
    """misalign: None, or which of the two pointers the predicate looks at ("qkv" / "da") sits one float past a 16-byte boundary."""
    __slots__ = ()

    @property
    def T(self):
        return self.H * self.W

    @property
    def branch(self):
        return branch(self.T, self.misalign is None)

    @property
    def id(self):
        return f"T{self.T}-{self.B}x{self.heads}x{self.H}x{self.W}" + (f"-{self.misalign}+4" if self.misalign else "")


def branch(T, aligned=True):
    """The branch launch_attention_bwd takes, as the suffix of its profiler row "attention_bwd_<branch>".  bwd_kernels.hip:1133:
    lds_path = T % 128 == 0 && ((qkv | da) & 15) == 0 (with MCEDM_ATTN_BWD_LDS at its default 1); :1135, and the launches at
    :1147-1161: otherwise T >= 128 -> <4>, T >= 64 -> <2>, else <1>."""
    if T % 128 == 0 and aligned:
        return "lds"
    return "direct<4>" if T >= 128 else ("direct<2>" if T >= 64 else "direct<1>")


def row(case):
    return "attention_bwd_" + case.branch


def _c(*rows, misalign=None):
    return [Case(*r, misalign) for r in rows]


# (B, heads, H, W): the smallest shapes at which each branch can still go wrong
CASES = (
    # direct<1>, T = 1, 31, 32, 33, 63: one token, a ragged single tile, one whole tile, one token into the second tile, two tiles
    _c((2, 1, 1, 1), (1, 2, 1, 31), (2, 1, 4, 8), (1, 1, 3, 11), (1, 2, 7, 9))
    # direct<2>, T = 65, 96, 100, 127: a ragged last tile on wave 0 (third tile: 65) or on wave 1 (fourth: 100, 127), two tiles per
    # wave; 96 is whole tiles with two on wave 0 and one on wave 1
    + _c((1, 2, 5, 13), (1, 2, 8, 12), (2, 2, 10, 10), (1, 1, 1, 127))
    # direct<4>, T = 129, 144, 169, 210, 240, 400, 529: the ragged last tile on wave 0 (129, 144, 400, 529: tile 4, 4, 12, 16), on
    # wave 1 (169: tile 5), 2 (210: tile 6) and 3 (240: tile 7); odd T, T % 4 != 0, up to five tiles per wave ...
    + _c((1, 1, 3, 43), (2, 2, 12, 12), (1, 1, 13, 13), (1, 2, 14, 15), (1, 2, 12, 20), (1, 1, 20, 20), (1, 1, 23, 23))
    # ... and whole tiles, where a caller's buffer is not 16-byte aligned
    + _c((2, 2, 8, 16), (4, 2, 16, 16), misalign="qkv") + _c((2, 2, 8, 16), (4, 2, 16, 16), misalign="da")
    # lds without the block remap (B heads % 8 != 0): T = 128, 384
    + _c((2, 2, 8, 16), (1, 1, 16, 24))
    # lds with it: B heads = 8 with 2, 3 and 4 workgroups per head; T = 512 also runs the forward attention_lds_kernel under the remap
    + _c((4, 2, 16, 16), (8, 1, 16, 24), (8, 1, 16, 32))
)

# plain     fx.randn
# spike     the key of the LAST token = 4 x the query of token 5 (score 32 against a spread of 4): the tile that the direct kernels
#           pad by clamping, and the LDS kernels' last chunk, holds the row maximum
# spike_kw  the same on key 32 (KW - 1) + 7, in the first tile of the last wave: the maximum moves in the cross-wave merge of the
#           statistics kernel, not in wave 0 (LDS kernels: in the fourth chunk, after three rescales)
# da50      da of the last token x 50
# x6        qkv x 6: scores of +-100 and more, softmax rows nearly one-hot
KINDS = ("plain", "spike", "spike_kw", "da50", "x6")


def kinds(case):
    """The kinds that exist for a case: the spikes need token 5, spike_kw more than one wave and its key inside T."""
    out = ["plain"]
    if case.T > 5:
        out.append("spike")
        if KW[case.branch] > 1 and spike_kw_key(case) < case.T - 1:
            out.append("spike_kw")
    return out + ["da50", "x6"]


def spike_kw_key(case):
    return 32 * (KW[case.branch] - 1) + 7


ALL = [(c, k) for c in CASES for k in kinds(c)]
IDS = [f"{c.id}-{k}" for c, k in ALL]


def packed_qkv(qkv, heads):
    B, C3, H, W = qkv.shape
    d = C3 // heads // 3
    return qkv.reshape(B, heads, d, 3, H, W).permute(0, 1, 3, 2, 4, 5).reshape(B, C3, H, W).contiguous()


def unpacked_qkv(p, heads):
    B, C3, H, W = p.shape
    d = C3 // heads // 3
    return p.reshape(B, heads, 3, d, H, W).permute(0, 1, 3, 2, 4, 5).reshape(B, C3, H, W).contiguous()


def _with_key(qkv, heads, key):
    B, C3, H, W = qkv.shape
    v = qkv.clone().reshape(B * heads, 64, 3, H * W)
    v[:, :, 1, key] = 4 * v[:, :, 0, 5]
    return v.reshape(B, C3, H, W)


def inputs(case, kind):
    """fp32 (qkv [B, heads 192, H, W] in the reference's channel order, da [B, heads 64, H, W]); the misaligned rows share the
    values of the aligned row of their shape."""
    B, heads, H, W = case[:4]
    qkv = fx.randn(f"{TAG}/{B}_{heads}_{H}_{W}/qkv", B, heads * 192, H, W)
    da = fx.randn(f"{TAG}/{B}_{heads}_{H}_{W}/da", B, heads * 64, H, W)
    if kind == "spike":
        qkv = _with_key(qkv, heads, case.T - 1)
    elif kind == "spike_kw":
        qkv = _with_key(qkv, heads, spike_kw_key(case))
    elif kind == "da50":
        da = da.clone()
        da.reshape(B, heads * 64, H * W)[:, :, -1] *= 50
    elif kind == "x6":
        qkv = qkv * 6
    else:
        assert kind == "plain", kind
    return qkv, da


def autograd(qkv, da, heads, dtype=torch.float64):
    """(a, dqkv) by autograd through the oracle in ``dtype``, in the reference's channel order."""
    x = qkv.to(dtype).requires_grad_(True)
    a = orc.attention(x, heads)
    (g,) = torch.autograd.grad(a, x, da.to(dtype))
    return a.detach(), g


@functools.lru_cache(maxsize=None)
def _reference(B, heads, H, W, kind):
    return autograd(*inputs(Case(B, heads, H, W, None), kind), heads)


def reference(case, kind):
    """The fp64 (a, dqkv) of a case, computed once and shared: do not write into them."""
    return _reference(*case[:4], kind)


def one_key_unmasked(case, kind="plain"):
    """The fp64 dqkv of a kernel that forgot to mask ONE padding key: the direct kernels load the keys past T clamped to the last
    token, so the mutant sees one more copy of it (with da = 0 on the copy, which as a query then contributes nothing).  Truncated
    to the T real tokens."""
    qkv, da = inputs(case, kind)
    B, heads, T = case.B, case.heads, case.T
    q = qkv.reshape(B, -1, 1, T)
    d = da.reshape(B, -1, 1, T)
    _, g = autograd(torch.cat([q, q[..., -1:]], -1), torch.cat([d, torch.zeros_like(d[..., -1:])], -1), heads)
    return g[..., :T].reshape(qkv.shape)
