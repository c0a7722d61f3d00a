"""What tools/make_golden_ddpm_arch.py (the reference's ``Model``, CPU) and the architecture tests of the DDPM U-Net share: the
table of networks, their parameters and inputs.  Everything here is regenerated from seeds and tags; only the reference's outputs
live in tests/golden/ddpm_arch.npz.

The table walks the family mcedm_ddpm_plan_create accepts -- any ch % 32 == 0, any ch_mult, 1 to 4 levels, any num_res_blocks,
attention wherever the width is 64 -- away from the one member every other test runs (ch 64, ch_mult (1, 1, 1), one block)."""
import dataclasses
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import ddpm_oracle as ddo  # noqa: E402
from oracle import fixtures as fx  # noqa: E402

B = 2
T_FWD = (3.0, 937.0)                     # an early timestep and a late one (large sin / cos arguments in the embedding)
SEED = 41
CPU_THREADS = 8                          # of the run that wrote the golden: an fp32 CPU conv is reproducible to the bit per thread count only


def _cfg(resolution, ch, ch_mult, num_res_blocks, attn_resolutions, channels=2, self_cond=True):
    return ddo.DdpmConfig(in_channels=channels, out_ch=channels, ch=ch, ch_mult=tuple(ch_mult), num_res_blocks=num_res_blocks,
                          attn_resolutions=tuple(attn_resolutions), resolution=resolution, self_cond=self_cond)


# tag -> configuration, ordered from the shipped shape outward.  What each reaches in csrc/ddpm.hip:
ARCHS = {
    # two attention blocks per level (256 tokens: the 4-way split kernel; 64 tokens), two skips pushed per level, parameter order
    "nrb2": _cfg(16, 64, (1, 1), 2, (16, 8)),
    # one level, no resampling; no self-conditioning channels (the n_self == 0 branch of conv_in)
    "one": _cfg(8, 64, (1,), 1, (8,), self_cond=False),
    # one state channel; 48^2 (Winograd: 48 % 16 == 0), 24^2 = 576-token mid attention in the LDS-staged kernel
    "r48": _cfg(48, 64, (1, 1), 1, (), channels=1),
    # a 128-channel level at 32^2 (quad records, 64 -> 128 shortcut as its own launch next to the Winograd conv2), 192-channel
    # concats of a quad- and a pair-record tensor in either order (table path), a 128-channel stride-2 conv
    "wide0": _cfg(32, 64, (2, 1), 1, (16,)),
    # 192-channel tensors (pair records), 256 = 192 + 64 concats fused from pair records under 8-channel groups
    "wide3": _cfg(32, 64, (3, 1), 1, (16,)),
    # 32-channel tensors (no records: table path), 96- and 32 + 32 concats, Cout = 32 convs, a 32 -> 64 shortcut in the down path,
    # the timestep kernel at ch = 32
    "narrow": _cfg(16, 32, (1, 2), 1, ()),
    # four levels of widths 32 / 64 / 128 / 64, attention over 16 tokens, up levels of unequal size (their re-numbering)
    "deep": _cfg(32, 32, (1, 2, 4, 2), 2, (4,)),
    # 2816 bias rows: the capped grid of the timestep kernel (64 workgroups of 44 rows); levels down to 2 x 2; 256 = 128 + 128
    # concats fused from quad records; a 128-channel up-sampling conv
    "rows3": _cfg(16, 64, (2, 2, 1, 1), 3, ()),
}
# the cond_enc / combine_enc head (mcedm_ddpm_plan_create_cond; cond_map + forward_cond)
HEADS = {
    "head_narrow3": dataclasses.replace(ARCHS["narrow"], cond_channels=3),        # one 32-channel chunk in the map kernel, R < its pixel block
    "head_r48": dataclasses.replace(ARCHS["r48"], cond_channels=1),               # R % 32 != 0: a partial pixel block
}
# cat_cond (forward_cat; self_cond False)
CATS = {
    "cat_one2": dataclasses.replace(ARCHS["one"], cond_channels=2, cat_cond=True),
    "cat_narrow1": dataclasses.replace(ARCHS["narrow"], self_cond=False, cond_channels=1, cat_cond=True),
}
ALL = {**ARCHS, **HEADS, **CATS}
# rows with a level of at least 32 x 32: the Winograd and the input-resident kernel families are in play
SWITCHED = ("wide0", "wide3", "r48")
# rows where some GroupNorm cannot be served from the producers' records (record_width: 32- and 96-channel tensors have none;
# a 192-channel concat of a quad- and a pair-record tensor has 6-channel groups) and takes a gn_coef_kernel pass
TABLE_PATH = {"narrow": True, "wide0": True, "deep": True, "rows3": True, "nrb2": False, "one": False, "wide3": False, "r48": False}


def params(tag, dtype=torch.float32):
    P = ddo.make_params(ALL[tag], SEED)
    return {k: v.to(dtype) for k, v in P.items()}


def inputs(tag):
    """x, x_self_cond (None without self-conditioning), cond (None without conditioning channels), NCHW fp32."""
    c = ALL[tag]
    R = c.resolution
    x = fx.randn(f"ddpma/{tag}/x", B, c.in_channels, R, R)
    xsc = fx.randn(f"ddpma/{tag}/xsc", B, c.in_channels, R, R) if c.self_cond else None
    cond = fx.randn(f"ddpma/{tag}/cond", B, c.cond_channels, R, R) if c.cond_channels else None
    return x, xsc, cond


def runs(tag):
    """(key, t, use x_self_cond, use cond) of every stored forward: both timesteps; a plain network with and without
    x_self_cond; a conditioned one with and without cond (x_self_cond given where the network takes one)."""
    c = ALL[tag]
    out = []
    for t in T_FWD:
        if c.cond_channels:
            out += [(f"{tag}::t{int(t)}::{'cond' if k else 'nocond'}", t, c.self_cond, k) for k in (True, False)]
        else:
            out += [(f"{tag}::t{int(t)}::{'sc' if s else 'nosc'}", t, s, False) for s in ((True, False) if c.self_cond else (False,))]
    return out


def oracle_forward(tag, P, key_run):
    _, t, use_sc, use_cond = key_run
    x, xsc, cond = inputs(tag)
    with torch.no_grad():
        return ddo.model_forward(P, ALL[tag], x, torch.full((B,), t), x_self_cond=xsc if use_sc else None,
                                 cond=cond if use_cond else None)


def attention_tokens(cfg):
    """Tokens of every attention block: down.L / up.L blocks work at resolution >> L, the middle block at the last level."""
    out = []
    for n, _ in ddo.param_shapes(cfg):
        if n.endswith(".q.weight"):
            level = len(cfg.ch_mult) - 1 if n.startswith("mid.") else int(n.split(".")[1])
            out.append((cfg.resolution >> level) ** 2)
    return out


def n_attention_blocks(cfg):
    return sum(n.endswith(".q.weight") for n, _ in ddo.param_shapes(cfg))


def make_plan(L, cfg):
    return L.DdpmPlan(cfg.in_channels, cfg.out_ch, cfg.ch, cfg.ch_mult, cfg.num_res_blocks, cfg.attn_resolutions, cfg.resolution,
                      self_cond=cfg.self_cond, cond_channels=cfg.cond_channels, cat_cond=cfg.cat_cond)


def bar_ratio(got, ref):
    """max over the entries of |got - ref| / (1e-5 max|ref| + 1e-4 |ref|): <= 1 is the project's bar (rtol 1e-4, atol 1e-5 max|ref|)."""
    got, ref = torch.as_tensor(got).detach().cpu().double(), torch.as_tensor(ref).double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float(((got - ref).abs() / (1e-5 * float(ref.abs().max()) + 1e-4 * ref.abs())).max())
