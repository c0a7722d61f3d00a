"""What tools/make_golden_adm_arch.py (the reference's ``DhariwalUNet``, CPU) and the architecture tests of the ADM U-Net share:
the table of networks, their parameters and inputs, the references in the dtype of the parameters, and what each row is expected
to launch.  Everything here is regenerated from seeds and tags; only the reference's outputs live in tests/golden/adm_arch.npz.

The table walks the family mcedm_unet_plan_create accepts -- any ch % 8 == 0, one to eight levels, any num_res_blocks, attention
wherever the width is a multiple of 64, any channel counts, any H, W that the levels divide -- away from the members every other
test runs (ch 64 / 128, square, 2 + 2 channels, one block per level, widths that are multiples of 32)."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import fixtures as fx  # noqa: E402
from oracle import mcedm_oracle as orc  # noqa: E402
from tests._ddpm_arch import bar_ratio  # noqa: E402,F401  (the project's bar: rtol 1e-4, atol 1e-5 max|ref|)

SEED = 43
CPU_THREADS = 8                          # of the run that wrote the golden: an fp32 CPU conv is reproducible to the bit per thread count only
LABEL = 0.3                              # the one broadcast noise label
SIGMAS = {2: (0.05, 30.0), 3: (0.05, 1.3, 30.0)}      # per-sample noise levels of the inference runs, by batch size


def _cfg(resolution, ch, ch_mult, attn=(), nrb=1, inc=2, cond=2, out=2):
    return orc.UNetConfig(in_channels=inc, cond_channels=cond, out_ch=out, ch=ch, ch_mult=tuple(ch_mult), num_res_blocks=nrb,
                          attn_resolutions=tuple(attn), resolution=resolution)


# tag -> (configuration, B, H, W).  What each is there to reach (conv_mfma.hip launch_conv, conv_wino.hip, norm_emb_attn.hip
# gn_sums_usable, plan.hip build_layout, backward.hip):
ARCHS = {
    # one level, no resampling block; four attention blocks at 8 x 8 x 64: the fused block in inference, not in training
    "one": (_cfg(8, 64, (1,), attn=(8,)), 3, 8, 8),
    # level 0 Winograd with three tile columns; level 1 at 16 x 24 (W % 16 != 0): neither Winograd form; concats 192 and 256,
    # 64 -> 128 skip projections
    "rect": (_cfg(32, 64, (1, 2)), 2, 32, 48),
    # no Winograd anywhere, ragged statistics tiles (ceil(H / 4) ceil(W / 8)), levels 6 x 10 and 3 x 5, attention over 15 tokens,
    # GroupNorm backward on 15-pixel planes
    "ragged": (_cfg(12, 64, (1, 1, 2), attn=(3,)), 2, 12, 20),
    # widths 80 and 40, concats 120 and 160 (5 channels per group), Cout % 32 != 0 throughout (padded weight tables), odd batch
    "narrow": (_cfg(16, 40, (2, 1)), 3, 16, 16),
    # widths 24 and 48; conv_in reads one channel with cond = NULL, out_conv writes 3; thin weight-gradient kernels; non-square
    "ch24": (_cfg(16, 24, (1, 2, 2), inc=1, cond=0, out=3), 2, 16, 32),
    # 192-wide level with 3-head attention at T = 256; concats 384 and 256; 6- and 12-channel groups; Winograd Cin 192 and 384
    "wide3": (_cfg(32, 64, (1, 3), attn=(16,)), 2, 32, 32),
    # five levels down to 2 x 2, 35 blocks, attention at T = 16 and T = 4, widths 32 to 128, two skips pushed per level
    "deep": (_cfg(32, 32, (1, 2, 2, 4, 2), attn=(4,), nrb=2), 2, 32, 32),
    # three blocks per level; images below 32 x 32 on whole 8 x 16 tiles (split Winograd in inference, not in training);
    # attention at T = 512 (2 heads) and T = 128
    "nrb3": (_cfg(16, 64, (2, 1), attn=(16,), nrb=3, inc=3, cond=1, out=3), 2, 16, 32),
    # Cout % 64 == 0 but not % 128 (the 64-channel Winograd configuration, three column blocks); T = 1024, 3 heads
    "c192": (_cfg(32, 192, (1,), attn=(32,)), 2, 32, 32),
    # attention at two levels; 256 -> 128 un-resampled skip projections that the folded Winograd epilogue takes; odd batch
    "c128a": (_cfg(32, 128, (1, 1), attn=(32, 16)), 3, 32, 32),
    # attention at token counts that are no multiple of 128 nor of 32: T = 400 (one head, three blocks) and T = 100 (two heads,
    # four blocks) -- in training the direct-from-global backward kernels with four and with two waves per tile (tests/_attn_bwd.py),
    # in inference a ragged attention_split_kernel<4> and attention_kernel; 20 x 20 and 10 x 10: no Winograd form anywhere
    "attn_rag": (_cfg(20, 64, (1, 2), attn=(20, 10)), 2, 20, 20),
}
# out_ch != in_channels: the EDM skip term c_skip x has no meaning; this row runs through forward / unet_backward under sum(w F^2)
PLAIN = ("ch24",)

# What the profiler rows of an INFERENCE call must show, per row, and the predicate each entry follows from:
#   wino   any conv_wino_kernel<WinoCfg<..>> / <WinoSkipCfg<..>> launch.  launch_conv takes conv_wino_applicable (Cout % 64 == 0,
#          H % 8 == 0, W % 16 == 0, Cin % 8 == 0) where conv_wino_preferred holds (H W >= 1024): the 32 x 48 and 32 x 32 levels of
#          widths 64 / 128 / 192, and in `deep` -- whose 32 x 32 level is 32 wide -- the 64 -> 64 convs of dec.32x32_up alone.
#   split  any conv_wino_kernel<WinoSplitCfg, ..> launch.  conv_wino_split_applicable: an un-resampled 3x3 conv on whole 8 x 16 tiles
#          below 1024 pixels with Cout % 32 == 0 and a Winograd table (place_conv: cout % 32 == 0, cin % 8 == 0): the 16 x 16 levels
#          of wide3 (192), deep (64) and c128a (128), the 16 x 32 and 8 x 16 levels of nrb3.  Not rect's 16 x 24, not the 80 / 40 /
#          24 / 48 wide convs of narrow and ch24, not 8 x 8 or smaller.
#   fold   any conv_wino_kernel<WinoSkipCfg<4>, ..> launch.  build_layout's wfold = conv_wino_fold_shape_ok: conv1 on the large
#          Winograd kernel, Cout % 128 == 0, a 32 .. 256 channel un-resampled projection in 16-channel halves: c128a's 256 -> 128
#          decoder blocks at 32 x 32 alone (rect, wide3: Cout 64; c192: Cout 192 and Cin 384).
#   table  any full-pass gn_coef_kernel launch.  gn_for_conv / launch_gn_coef_from_sums fall back to it where gn_sums_usable fails:
#          the ADM executor's records hold 4 channels, so a GroupNorm whose groups are not whole records -- 5 channels per group at
#          160, 6 at 192 -- has none.  192 = 128 + 64 (rect, ragged, deep, nrb3, attn_rag) or a level width (wide3, c192); 160 = 80 + 80
#          (narrow).  one (64, 128), ch24 (24, 48, 72, 96: 4 per group) and c128a (128, 256) never need it.
PATHS = {
    "one": dict(wino=False, split=False, fold=False, table=False),
    "rect": dict(wino=True, split=False, fold=False, table=True),
    "ragged": dict(wino=False, split=False, fold=False, table=True),
    "narrow": dict(wino=False, split=False, fold=False, table=True),
    "ch24": dict(wino=False, split=False, fold=False, table=False),
    "wide3": dict(wino=True, split=True, fold=False, table=True),
    "deep": dict(wino=True, split=True, fold=False, table=True),
    "nrb3": dict(wino=False, split=True, fold=False, table=True),
    "c192": dict(wino=True, split=False, fold=False, table=True),
    "c128a": dict(wino=True, split=True, fold=True, table=False),
    "attn_rag": dict(wino=False, split=False, fold=False, table=True),
}
# attention: launch_attention (attention_kernel) once per attention block, except where run_block takes
# attn_block_fused_applicable (C == 64, one head, 8 x 8, inference: `one`): then attn_block64_kernel, and attention_kernel 0
FUSED_ATTN = ("one",)
# backward: wgrad_thin_applicable serves the 3x3 convs with at most 4 channels on one side and at least 16 on the other, one
# wgrad_thin*_kernel launch each: out_conv (24 -> 3) of ch24; conv_in (1 + 3 -> 128) and out_conv (64 -> 3) of nrb3.  NOT ch24's
# conv_in (1 -> 24): a thin INPUT must arrive as the first source (`thin_in && a.xa == nullptr` is refused), and without
# conditioning channels conv_in's one channel is the second source of cat(cond, x); it takes the direct kernel
THIN_WGRADS = {"ch24": 1, "nrb3": 2}
# backward: wgrad_wino_kernel where wgw_form_of gives the 128-channel form (Cout % 128 == 0, Cin % 128 == 0, W % 32 == 0): the
# 128 -> 128 and 256 -> 128 convs of c128a's 32 x 32 level
WGRAD_WINO = ("c128a",)
# kernel family switched off on the plan alone -> (rows it is run on, the prefix its launches carry in the profiler rows).
# (conv1x1_reg: try_launch_conv1x1_reg leaves 64-channel projections below 4096 pixels to the resident kernels -- rect's 192 -> 64
# and 128 -> 64 at 32 x 48 -- and c128a's 256 -> 128 projections ride on the fold; in inference it launches on c128a with the
# fold off, which test_hip_adm_arch.py asserts, and both off is a case of its own there)
SWITCHED = {
    "conv_wino": (("rect", "wide3", "c192", "c128a"), "conv_wino"),
    "conv_resident": (("ragged", "narrow", "deep"), "conv_resident"),
    "conv_wino_split": (("nrb3",), "conv_wino_kernel<WinoSplitCfg"),
    "conv_wino_fold": (("c128a",), "conv_wino_kernel<WinoSkipCfg"),
    "conv1x1_reg": (("rect", "c128a"), "conv1x1_reg"),
    "attn_fused": (("one",), "attn_block64"),
}
SWITCHED_TRAINING = {"wgrad_wino": (("wide3", "c128a"), "wgrad_wino")}


def cfg_of(tag):
    return ARCHS[tag][0]


def params(tag, dtype=torch.float32):
    return orc.make_params(cfg_of(tag), SEED, dtype=dtype)


def inputs(tag):
    """fp32, NCHW: x, cond (None without conditioning channels), mask, noise, rnd_normal [B, 1, 1, 1] of the training step, and
    sigma [B] of the inference runs (0.05 to 30)."""
    c, B, H, W = ARCHS[tag]
    x = fx.randn(f"adma/{tag}/x", B, c.in_channels, H, W)
    cond = fx.randn(f"adma/{tag}/cond", B, c.cond_channels, H, W) if c.cond_channels else None
    mask = torch.zeros(B, c.in_channels, H, W)
    mask[0, -1] = 1
    mask[1, 0] = 1
    mask[1, -1, : H // 2] = 1
    if B > 2:
        mask[2, :, :, W // 3:] = 1
    noise = fx.randn(f"adma/{tag}/noise", B, c.in_channels, H, W)
    rnd_normal = fx.randn(f"adma/{tag}/rnd", B, 1, 1, 1)
    return dict(x=x, cond=cond, mask=mask, noise=noise, rnd_normal=rnd_normal, sigma=torch.tensor(SIGMAS[B], dtype=torch.float32))


def loss_weights(tag):
    """w of the plain row's loss sum(w F^2): positive, of the output's shape."""
    c, B, H, W = ARCHS[tag]
    return 0.5 + fx.randn(f"adma/{tag}/w", B, c.out_ch, H, W).abs()


def runs(tag):
    """(key, kind) of every stored forward: per-sample noise levels, one broadcast label, and cond = None where the row has
    conditioning channels."""
    out = [(f"{tag}::F_sigma", "sigma"), (f"{tag}::F_label", "label")]
    if cfg_of(tag).cond_channels:
        out.append((f"{tag}::F_nocond", "nocond"))
    return out


def grad_names(tag):
    """The three small tensors whose full gradients are stored: the first conv's bias, one affine.bias, out_conv.weight."""
    c = cfg_of(tag)
    r = c.resolution >> (len(c.ch_mult) - 1)
    return [f"enc.{c.resolution}x{c.resolution}_conv.bias", f"dec.{r}x{r}_in0.affine.bias", "out_conv.weight"]


def golden_keys(tag):
    return [k for k, _ in runs(tag)] + [f"{tag}::loss", f"{tag}::grad_sqnorm_each"] + [f"{tag}::grad::{n}" for n in grad_names(tag)]


def _network(P, tag, net):
    if net is not None:
        return net
    c = cfg_of(tag)
    return lambda x, labels, cond: orc.unet_forward(P, c, x, labels, cond)


def denoise_ref(tag, P, kind, net=None):
    """One stored run in the dtype of P -> (D, F); D is None for the plain row and for the label runs.  'sigma': preconditioning
    (orc.precond_coeffs on sigma in P's dtype) around the network, one noise level per sample -- the plain row feeds ln(sigma) / 4
    as labels and x as it is.  'label' / 'nocond': the network on x with the one broadcast label, cond given / None.
    net: (x, labels, cond) -> F stands in for orc.unet_forward (the generator passes the reference network)."""
    dt = next(iter(P.values())).dtype
    f = _network(P, tag, net)
    I = inputs(tag)
    x = I["x"].to(dt)
    cond = None if I["cond"] is None else I["cond"].to(dt)
    with torch.no_grad():
        if kind != "sigma":
            return None, f(x, torch.tensor([LABEL], dtype=torch.float32).to(dt), cond if kind == "label" else None)
        sigma = I["sigma"].double().to(dt).reshape(-1, 1, 1, 1)
        c_skip, c_out, c_in, c_noise = orc.precond_coeffs(sigma)
        if tag in PLAIN:
            return None, f(x, c_noise.flatten(), cond)
        F = f(c_in * x, c_noise.flatten(), cond)
        return c_skip * x + c_out * F, F


def training_ref(tag, P, net=None):
    """The training step in the dtype of P -> the loss (a tensor that carries the graph; P or net's parameters must require grad).
    EDM rows: the masked EDM loss of PlMcedm.training_step (orc.training_loss's formula on orc.precond_coeffs / orc.loss_weight,
    sigma in P's dtype).  The plain row: sum(w F^2) of the network at per-sample labels ln(sigma) / 4."""
    dt = next(iter(P.values())).dtype
    f = _network(P, tag, net)
    I = inputs(tag)
    x = I["x"].to(dt)
    cond = None if I["cond"] is None else I["cond"].to(dt)
    if tag in PLAIN:
        labels = plain_labels(tag).to(dt)
        return (loss_weights(tag).to(dt) * f(x, labels, cond) ** 2).sum()
    mask, noise = I["mask"].to(dt), I["noise"].to(dt)
    sigma = (I["rnd_normal"].double().to(dt) * orc.P_STD + orc.P_MEAN).exp()
    weight = orc.loss_weight(sigma)
    x_noise = x + mask * noise * sigma
    c_skip, c_out, c_in, c_noise = orc.precond_coeffs(sigma)
    D = c_skip * x_noise + c_out * f(c_in * x_noise, c_noise.flatten(), cond)
    return (weight * (D * mask - x * mask) ** 2).sum(dim=(1, 2, 3)).mean()


def plain_labels(tag):
    """fp32 [B] noise labels of the plain row's training step: ln(sigma) / 4 of the inference noise levels."""
    return orc.precond_coeffs(inputs(tag)["sigma"])[3]


def training_grads(tag, dtype=torch.float64):
    """(loss, name -> gradient) by autograd through the oracle in ``dtype``."""
    P = {k: v.requires_grad_(True) for k, v in params(tag, dtype).items()}
    loss = training_ref(tag, P)
    grads = torch.autograd.grad(loss, list(P.values()))
    return loss.detach(), dict(zip(P, grads))


def attention_tokens(tag):
    """Tokens of each attention block of the row, in execution order."""
    c, _, H, W = ARCHS[tag]
    spec = orc.build_spec(c)
    out = []
    for b in spec.enc + spec.dec:
        res = int(b.key.split(".")[1].split("x")[0])
        level = (c.resolution // res).bit_length() - 1
        if b.attn:
            out.append((H >> level) * (W >> level))
    return out


def gn_widths(tag):
    """{C: channels per group} of every GroupNorm of the row (adm_blocks.py:86-97: groups = min(32, C // 4))."""
    return {s[0]: s[0] // min(32, s[0] // 4) for n, s in orc.param_shapes(cfg_of(tag)) if ".norm" in n or n.startswith("out_norm")}


def level_sizes(tag):
    c, _, H, W = ARCHS[tag]
    return [(H >> lv, W >> lv, c.ch * m) for lv, m in enumerate(c.ch_mult)]


def make_plan(L, cfg):
    return L.Plan(cfg.in_channels, cfg.cond_channels, cfg.out_ch, cfg.ch, cfg.ch_mult, cfg.num_res_blocks, cfg.attn_resolutions,
                  cfg.resolution)
