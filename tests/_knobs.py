"""The environment knobs of the HIP library (csrc: `static const int v = env_int("MCEDM_...", d)`, INTEGRATION.md "Environment
switches") select kernels, template instantiations and shapes that the default process never reaches.  Each is read once per
process, so a variant runs in a child process of its own: run as a program (python tests/_knobs.py GROUP OUT.npz) this file IS
the child -- it reads no knob itself, the parent sets the environment; it computes and stores, and every comparison happens in the
parent (tests/test_hip_knobs.py).  tests/test_knobs_cpu.py holds the tables to the branches and edges they claim.  Nothing here
needs a GPU to import.

    GROUPS              name -> (environment, case keys): one group = one child process
    CASES               key -> Case(kind, shape ..., the profiler rows it must and must not show)
    COVERED_ELSEWHERE   knob -> (test file, test function) that already sets it
    EXCLUDED            knob -> (reason, test file, test function or None)

Also the inputs, fp64 references and device runs of the GroupNorm backward and the register-direct 1x1 conv, shared with
tests/test_hip_backward.py and tests/test_hip_conv1x1.py.

Attention shapes are (B, heads, H, W) with inputs and the fp64 reference of tests/_attn_bwd.py; kinds plain, spike (the last key
holds the row maximum) and x6 (scores of +-100: where a backward that recomputes its probabilities in other units than the
forward formed them leaves the bar)."""
import collections
import functools
import importlib
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import fixtures as fx  # noqa: E402
from oracle import mcedm_oracle as orc  # noqa: E402
from tests import _attn_bwd as AB  # noqa: E402

# ---------------------------------------------------------------------------------------------------------------------------------
# the launchers' predicates, restated


def attn_fwd_row(T, env=None, aligned=True):
    """The profiler row of launch_attention with its variant, "attention_kernel[<variant>]" (csrc/norm_emb_attn.hip:667), i.e. common.hpp:71-79 attn_fwd_kernel: mode =
    MCEDM_ATTN_SPLIT (1), lds_min = MCEDM_ATTN_LDS_MIN (512); aligned = T % 4 == 0 and qkv 16-byte aligned.
    mode >= 1 and mode != 2 and T >= lds_min and aligned -> lds<1> (mode 3) / lds<2>; else mode and T >= 256 -> split<4>; else
    mode and T >= 128 -> split<2>; else one."""
    env = env or {}
    mode, lds_min = int(env.get("MCEDM_ATTN_SPLIT", 1)), int(env.get("MCEDM_ATTN_LDS_MIN", 512))
    al = aligned and T % 4 == 0
    if mode >= 1 and mode != 2 and T >= lds_min and al:
        return "attention_kernel[lds<1>]" if mode == 3 else "attention_kernel[lds<2>]"
    if mode and T >= 256:
        return "attention_kernel[split<4>]"
    if mode and T >= 128:
        return "attention_kernel[split<2>]"
    return "attention_kernel[one]"


def attn_fwd_variant(T, env=None, aligned=True):
    """The variant alone: one, split<2>, split<4>, lds<1> or lds<2>."""
    return attn_fwd_row(T, env, aligned)[len("attention_kernel["):-1]


def attn_fwd_base2(T, env=None, aligned=True):
    """common.hpp:81: only attention_kernel forms its scores in natural units."""
    return attn_fwd_row(T, env, aligned) != "attention_kernel[one]"


def attn_bwd_row(T, env=None, aligned=True):
    """The profiler row of launch_attention_bwd (csrc/bwd_kernels.hip:1132-1135): lds where MCEDM_ATTN_BWD_LDS (1) and T % 128 == 0
    and qkv, da 16-byte aligned; else direct<4> from 128, direct<2> from 64 tokens, else direct<1>."""
    env = env or {}
    if int(env.get("MCEDM_ATTN_BWD_LDS", 1)) and T % 128 == 0 and aligned:
        return "attention_bwd_lds"
    return "attention_bwd_" + ("direct<4>" if T >= 128 else "direct<2>" if T >= 64 else "direct<1>")


def gn_groups(C):
    return min(32, C // 4)


def gn_reg_quads(case):
    """gn_bwd_reg_plan (csrc/bwd_kernels.hip:503-517) without its switch -> (quads per thread R or 0, lanes per channel)."""
    B, Ca, Cb, Hs, Ws, rs = case[:6]
    C = Ca + Cb
    cpg, hw = C // gn_groups(C), Hs * Ws
    if rs != 0 or hw % 4 or cpg * hw > 8192:
        return 0, 0
    hw4 = hw // 4
    if hw4 >= 64:
        if hw4 % 64:
            return 0, 0
        seg = 64
    else:
        if hw4 < 16 or hw4 & (hw4 - 1):
            return 0, 0
        seg = hw4
    q = cpg * hw4
    return (1 if q <= 256 else 2 if q <= 512 else 4 if q <= 1024 else 8), seg


def gn_lds_served(case):
    """gn_bwd_lds_plan (csrc/bwd_kernels.hip:376-388) without its switch, for aligned buffers: a `sync` buffer, whole pieces of
    4096 elements, slabs of >= 16384, resampled sources with Ws % 4 == 0 and even Hs."""
    B, Ca, Cb, Hs, Ws, rs = case[:6]
    C = Ca + Cb
    cpg, hw = C // gn_groups(C), Hs * Ws
    if len(case) <= 10 or hw % 4096 or cpg * hw < 16384:
        return False
    return rs == 0 or (Ws % 4 == 0 and Hs % 2 == 0)


def gn_bwd_row(case, env=None):
    """The profiler row of launch_gn_bwd (csrc/bwd_kernels.hip:519-551): the LDS-resident kernel (MCEDM_GN_BWD_LDS, 1), else the
    register kernel (MCEDM_GN_BWD_REG, 1), else the two-pass kernel: <1024> where MCEDM_GN_BWD_NT is 1024 (its default) and the
    slab has >= 16384 elements, else <256>."""
    env = env or {}
    B, Ca, Cb, Hs, Ws = case[:5]
    C = Ca + Cb
    if int(env.get("MCEDM_GN_BWD_LDS", 1)) and gn_lds_served(case):
        return "gn_bwd_lds_kernel"
    if int(env.get("MCEDM_GN_BWD_REG", 1)) and gn_reg_quads(case)[0]:
        return "gn_bwd_reg_kernel"
    big = int(env.get("MCEDM_GN_BWD_NT", 1024)) == 1024 and C // gn_groups(C) * Hs * Ws >= 16384
    return "gn_bwd_kernel[<1024>]" if big else "gn_bwd_kernel[<256>]"


def c1_row(Cout, env=None):
    """try_launch_conv1x1_reg (csrc/conv1x1_reg.hip:174, 210-219): <NI, MT>, MT = 128 where Cout % 128 == 0 else 64 (NI = 2 only);
    NI = MCEDM_C1_NI (2): anything but 2 is 4."""
    if Cout % 128:
        return "conv1x1_reg_kernel[<2, 64>]"
    return "conv1x1_reg_kernel[<2, 128>]" if int((env or {}).get("MCEDM_C1_NI", 2)) == 2 else "conv1x1_reg_kernel[<4, 128>]"


# ---------------------------------------------------------------------------------------------------------------------------------
# cases

# kind: attn_fwd (shape = (B, heads, H, W), sub = input kind), attn_pair (forward of this process, then the backward), c1 (shape =
# (B, Ca, Cb, Cout, H, W, use_res)), gn (shape = the case tuple of test_gn_film_silu_backward).  must / must_not: profiler rows;
# an entry that ends in "*" is a prefix.  wino: shape = (B, Ca, Cb, Cout, H, W).
Case = collections.namedtuple("Case", "kind shape sub must must_not")
CASES = {}
GROUPS = {}

ATTN_SHAPE = {
    128: (2, 2, 8, 16), 129: (1, 1, 3, 43), 130: (1, 1, 10, 13), 132: (1, 2, 11, 12), 160: (1, 1, 10, 16), 169: (1, 1, 13, 13),
    192: (1, 1, 12, 16), 256: (4, 2, 16, 16), 384: (1, 1, 16, 24), 512: (1, 2, 16, 32), 516: (1, 1, 12, 43), 529: (1, 1, 23, 23),
    544: (1, 1, 16, 34), 576: (1, 1, 24, 24), 640: (2, 1, 20, 32),
}
ATTN_KINDS = ("plain", "spike", "x6")
# Every shape is one on which an fp32 sum of the scores meets the bar in BOTH unit systems (tests/test_knobs_cpu.py
# test_the_bar_is_fair_to_fp32_attention).  T = 256 was (1, 2, 16, 16) at first: there the x6 forward in units of log 2 -- the
# DEFAULT path's split<4>, and lds<2> under MCEDM_ATTN_LDS_MIN -- measured 1.0930 of the bar on `a` on an MI355X, to four digits
# what a plain fp32 sum of q log2(e) / 8 . k gives on the CPU (natural units: 0.5977, kernel and CPU alike).  The rounding of a
# score of +-200 is 1.5e-5 whatever the kernel does with it afterwards, so the input was changed, not the bar.


ATTN_FWD_VARIANTS = ("one", "split<2>", "split<4>", "lds<1>", "lds<2>")
ATTN_BWD_SUFFIX = ("bwd_lds", "bwd_direct<1>", "bwd_direct<2>", "bwd_direct<4>")
ATTN_ROWS = tuple(f"attention_kernel[{v}]" for v in ATTN_FWD_VARIANTS) + tuple("attention_" + s for s in ATTN_BWD_SUFFIX)


def _group(name, env):
    GROUPS[name] = (dict(env), [])
    return GROUPS[name]


def _attn(group, T, kinds=ATTN_KINDS, pair=False, shape=None):
    env, keys = GROUPS[group]
    shape = shape or ATTN_SHAPE[T]
    assert shape[2] * shape[3] == T
    rows = (attn_fwd_row(T, env),) + ((attn_bwd_row(T, env),) if pair else ())
    for k in kinds:
        key = f"{group}/{'pair' if pair else 'fwd'}/T{T}/{k}"
        CASES[key] = Case("attn_pair" if pair else "attn_fwd", shape, k, rows, tuple(r for r in ATTN_ROWS if r not in rows))
        keys.append(key)


# attn_split0: attention_kernel above 127 tokens, 4 to 17 key tiles on ONE wave, the ragged last tile at 169 and 529; the
# backward pairs are the finding of this table: the backward recomputed its probabilities in units of log 2 from 128 tokens on
# while this forward forms them in natural units (T = 129, 169: direct<4>; 256, 512: the LDS kernels).  Their shapes are the ones at
# which a model of that mismatch leaves the bar (tests/test_knobs_cpu.py: 1.2 at 169, 1.6 at 256; at 129 no batch up to 16 heads
# does, 0.91: the T = 129 pair therefore only holds the fixed path (direct<4> in natural units, a ragged tile) to fp64 and would
# not have caught the bug -- the unfixed kernel measured 0.93 there; 169, 256 and 512 catch it, 512 added for that)
_group("attn_split0", {"MCEDM_ATTN_SPLIT": "0"})
for _T in (128, 169, 256, 512, 529):
    _attn("attn_split0", _T)
SPLIT0_PAIRS = {129: (4, 2, 3, 43), 169: (4, 2, 13, 13), 256: (4, 2, 16, 16), 512: (1, 2, 16, 32)}
for _T, _s in SPLIT0_PAIRS.items():
    _attn("attn_split0", _T, kinds=("x6",), pair=True, shape=_s)
# attn_split2: split<4> past the LDS threshold: 16, 18 and 20 key tiles = 4 / 4 / 4 / 4, 5 / 5 / 4 / 4 and 5 / 5 / 5 / 5 per wave (the merge
# of waves with unequal tile counts); the direct<4> backward on aligned whole tiles
_group("attn_split2", {"MCEDM_ATTN_SPLIT": "2", "MCEDM_ATTN_BWD_LDS": "0"})
for _T in (512, 576, 640):
    _attn("attn_split2", _T)
for _T in (128, 256, 384, 512):
    _attn("attn_split2", _T, pair=True)
# attn_lds1: the four-wave LDS kernel (32-key staged tiles): 516 = 12 x 43 has 4 keys in its last tile and a ragged query
# block (four query tiles of 32 + 4 tokens in the fifth workgroup), 544 a whole last tile and one query tile in the last
# workgroup; 529 is odd and stays on split<4>
_group("attn_lds1", {"MCEDM_ATTN_SPLIT": "3"})
for _T in (512, 516, 544, 640, 529):
    _attn("attn_lds1", _T)
# attn_ldsmin: the eight-wave LDS kernel (64-key staged tiles) on 2 to 4 staged tiles: 128 = two tiles, no prefetch after the
# first; at 132 and 160 the odd half of the last staged tile ([128 + 32, 128 + 64)) lies wholly past T: waves 4..7 see a tile of
# -inf scores and must add nothing to what they hold (their first tile lies inside T, so their running maximum is finite: the
# m_new > -inf and a1 guards themselves fire only below 33 tokens); 130 is not a multiple of 4: split<2>
_group("attn_ldsmin", {"MCEDM_ATTN_LDS_MIN": "128"})
for _T in (128, 132, 160, 192, 256, 130):
    _attn("attn_ldsmin", _T)
for _T in (132, 256):
    _attn("attn_ldsmin", _T, kinds=("x6",), pair=True)
# attn_ldsmin16: what 132 and 160 do not reach.  With ONE staged tile of 64 keys and T <= 32 the odd half lies wholly past T on
# the FIRST tile of waves 4..7: their running maximum stays -inf (the `m_new > -INFINITY` guard, norm_emb_attn.hip:589) and the
# merge must take nothing from them (the `a1` guard, :631); T = 16, 20 (ragged even half) and 32 (whole even half).  The pair at
# 32 runs attn_bwd_*_kernel<1, true>: one wave per tile in units of log 2, which no default path instantiates
_group("attn_ldsmin16", {"MCEDM_ATTN_LDS_MIN": "16"})
LDSMIN16_SHAPE = {16: (2, 2, 4, 4), 20: (1, 2, 4, 5), 32: (2, 1, 4, 8)}
for _T, _s in LDSMIN16_SHAPE.items():
    _attn("attn_ldsmin16", _T, shape=_s)
_attn("attn_ldsmin16", 32, kinds=("x6",), pair=True, shape=LDSMIN16_SHAPE[32])
# attn_xcd0: workgroups in dispatch order where the default remaps them (B heads % 8 == 0): the same bits
XCD_FWD, XCD_BWD = (4, 2, 16, 32), (4, 2, 16, 16)
_group("attn_xcd0", {"MCEDM_ATTN_XCD": "0"})
_attn("attn_xcd0", 512, shape=XCD_FWD)
_attn("attn_xcd0", 256, pair=True, shape=XCD_BWD)

# c1_ni4: conv1x1_reg_kernel<4>: all 128 output channels per wave, 8-byte loads.  (B, Ca, Cb, Cout, H, W, use_res).  Cin = 16
# is ONE stage (the reload of the last stage, the dropped one, is then the only reload), Cin = 16 + 32 three stages from two
# tensors; 5 x 2 tiles on 256 workgroups' worth of grid; Cout = 256: two output-channel blocks
C1_CASES = [(2, 128, 128, 128, 32, 32, False), (3, 64, 0, 128, 32, 32, True), (1, 16, 0, 128, 32, 32, False),
            (1, 16, 32, 128, 16, 64, True), (5, 256, 0, 128, 32, 32, False), (2, 128, 0, 256, 32, 32, False)]
_group("c1_ni4", {"MCEDM_C1_NI": "4"})


def c1_key(shape):
    return "c1/" + "_".join(map(str, shape[:6])) + ("_res" if shape[6] else "")


for _s in C1_CASES:
    CASES["c1_ni4/" + c1_key(_s)] = Case("c1", _s, None, (c1_row(_s[3], GROUPS["c1_ni4"][0]),), ("conv1x1_reg_kernel[<2, 128>]", "conv1x1_reg_kernel[<2, 64>]"))
    GROUPS["c1_ni4"][1].append("c1_ni4/" + c1_key(_s))

# gn_twopass: the two-pass kernel on the shapes the register and the LDS-resident kernel serve by default.
# (B, Ca, Cb, Hs, Ws, resample, act, film, add_mode, accumulate[, "sync"]) as test_gn_film_silu_backward
GN_CASES = [
    (2, 64, 0, 8, 8, 0, 1, True, 0, False),              # register kernel: 1 quad per thread, 16 lanes per channel
    (2, 16, 0, 16, 16, 0, 1, False, 0, False),           # 1 quad, 64 lanes per channel
    (2, 64, 64, 16, 32, 0, 1, False, 1, True),           # 2 quads, two input tensors
    (2, 128, 0, 32, 32, 0, 1, True, 1, False),           # 4 quads
    (1, 64, 0, 32, 64, 0, 0, True, 0, False),            # 8 quads
    (2, 64, 64, 64, 64, 0, 0, False, 1, True, "sync"),   # the smallest LDS-resident shape: slabs of 16384 elements
    (2, 128, 0, 64, 64, 1, 1, False, 2, True, "sync"),   # resampled: the gradient comes back through the 2x up-sampling ...
    (1, 128, 0, 64, 64, 2, 1, False, 1, False, "sync"),  # ... and through the 2 x 2 mean
]
GN_ROWS = ("gn_bwd_lds_kernel", "gn_bwd_reg_kernel", "gn_bwd_kernel[<256>]", "gn_bwd_kernel[<1024>]")
_group("gn_twopass256", {"MCEDM_GN_BWD_LDS": "0", "MCEDM_GN_BWD_REG": "0", "MCEDM_GN_BWD_NT": "256"})
_group("gn_twopass1024", {"MCEDM_GN_BWD_LDS": "0", "MCEDM_GN_BWD_REG": "0"})


def gn_key(case):
    return "gn/" + "_".join(map(str, case))


for _g in ("gn_twopass256", "gn_twopass1024"):
    for _c in GN_CASES:
        _row = gn_bwd_row(_c, GROUPS[_g][0])
        CASES[f"{_g}/{gn_key(_c)}"] = Case("gn", _c, None, (_row,), tuple(r for r in GN_ROWS if r != _row))
        GROUPS[_g][1].append(f"{_g}/{gn_key(_c)}")

# wino_min256: the large Winograd kernel (WinoCfg<2> / WinoCfg<4>, one 8 x 16 tile per workgroup) at 16 x 16 and 16 x 32 through the
# dispatcher, where the default threshold of 1024 pixels sends the split form.  (B, Ca, Cb, Cout, H, W).  8 x 16 = 128 pixels is
# below 256 too: conv_wino_small() still holds, so the dispatcher (conv_mfma.hip:890-893) gives it to the split form as by default
# -- it must not show the large kernel
WINO_CASES = [(2, 64, 0, 64, 16, 16), (1, 128, 128, 128, 16, 16), (2, 64, 0, 128, 16, 32), (2, 64, 0, 64, 8, 16)]
WINO_LARGE, WINO_SPLIT = "conv_wino_kernel<WinoCfg<*", "conv_wino_kernel<WinoSplitCfg*"
_group("wino_min256", {"MCEDM_WINO_MIN_HW": "256"})


def wino_row(shape, env=None):
    """The dispatcher's choice for an un-resampled 3x3 conv with a Winograd table on whole 8 x 16 tiles (conv_mfma.hip:890-893,
    conv_wino.hip:1293-1296): the large kernel from MCEDM_WINO_MIN_HW (1024) pixels on, below it the split form."""
    return WINO_LARGE if shape[4] * shape[5] >= int((env or {}).get("MCEDM_WINO_MIN_HW", 1024)) else WINO_SPLIT


def wino_key(shape):
    return "wino/" + "_".join(map(str, shape))


for _s in WINO_CASES:
    _row = wino_row(_s, GROUPS["wino_min256"][0])
    CASES["wino_min256/" + wino_key(_s)] = Case("wino", _s, None, (_row,), tuple(r for r in (WINO_LARGE, WINO_SPLIT) if r != _row))
    GROUPS["wino_min256"][1].append("wino_min256/" + wino_key(_s))

COVERED_ELSEWHERE = {
    "MCEDM_WINO_PER": ("tests/test_hip_wino_per.py", "test_forced_tiles_per_workgroup_vs_fp64_and_bit_equal_to_one_tile"),
    "MCEDM_WINO_MAP": ("tests/test_hip_wino.py", "test_interleaved_tile_map_is_bit_identical_to_consecutive_tiles"),
    "MCEDM_GN_BWD_SPIN_US": ("tests/test_hip_backward.py", "test_gn_backward_partner_wait_timeout_gives_the_same_bits"),
}
# knob -> (reason, the test that runs the fallback kernel at such a shape: file, function -- or None, None)
EXCLUDED = {
    "MCEDM_WINO_MODE": ("unused outside the -DMCEDM_WINO_TIMELINE build", None, None),
    "MCEDM_CONV_EXTRA_LDS": ("an occupancy diagnostic: unused dynamic LDS, no arithmetic changes", None, None),
    "MCEDM_RES_BIG": ("0 leaves the >= 64 x 64 one-tile convs on conv_mfma_kernel's <64, 8, 32> tile, which runs at 64 x 64 there",
                      "tests/test_hip_parity.py", "test_conv_every_tile_configuration"),
}

# ---------------------------------------------------------------------------------------------------------------------------------
# inputs and fp64 references


def attn_case(shape):
    return AB.Case(*shape, None)


def attn_reference(shape, kind):
    """fp64 (a, dqkv) in the reference's channel order (tests/_attn_bwd.py reference: computed once, shared)."""
    return AB.reference(attn_case(shape), kind)


def c1_inputs(shape):
    """The inputs of tests/test_hip_conv1x1.py for (B, Ca, Cb, Cout, H, W, use_res)."""
    B, Ca, Cb, Cout, H, W, use_res = shape
    tag, Cin = f"c1/{B}_{Ca}_{Cb}_{Cout}_{H}_{W}", Ca + Cb
    return dict(xa=fx.randn(tag + "/xa", B, Ca, H, W), xb=fx.randn(tag + "/xb", B, Cb, H, W) if Cb else None,
                w=fx.randn(tag + "/w", Cout, Cin, 1, 1) / Cin ** 0.5, b=fx.randn(tag + "/b", Cout) * 0.1,
                res=fx.randn(tag + "/r", B, Cout, H, W) if use_res else None)


def c1_reference(t, dtype=torch.float64):
    x = torch.cat([t["xa"], t["xb"]], 1) if t["xb"] is not None else t["xa"]
    ref = F.conv2d(x.to(dtype), t["w"].to(dtype), t["b"].to(dtype))
    return ref + t["res"].to(dtype) if t["res"] is not None else ref


def wino_inputs(shape):
    B, Ca, Cb, Cout, H, W = shape
    tag, Cin = "knobs/" + wino_key(shape), Ca + Cb
    return dict(xa=fx.randn(tag + "/xa", B, Ca, H, W), xb=fx.randn(tag + "/xb", B, Cb, H, W) if Cb else None,
                w=fx.randn(tag + "/w", Cout, Cin, 3, 3) / (Cin * 9) ** 0.5, b=fx.randn(tag + "/b", Cout) * 0.1)


def wino_reference(t, dtype=torch.float64):
    x = torch.cat([t["xa"], t["xb"]], 1) if t["xb"] is not None else t["xa"]
    return F.conv2d(x.to(dtype), t["w"].to(dtype), t["b"].to(dtype), padding=1)


@functools.lru_cache(maxsize=None)
def wino_reference64(shape):
    return wino_reference(wino_inputs(shape))


def run_wino(L, shape, t):
    """A 3x3 conv with a Winograd table through the dispatcher, as a plan launches it -> (out, profiler rows)."""
    w, b = dev(t["w"]), dev(t["b"])
    wpk, bpk = L.op_pack_conv(w, b)
    wino = L.op_pack_conv_wino(w)
    xa, xb = dev(t["xa"]), dev(t["xb"])
    return profiled(L, lambda: L.op_conv_sums(xa, xb, wpk, bpk, shape[3], 3, wino=wino)[0])


def gn_inputs(case):
    """The fp32 inputs of a GroupNorm / FiLM / SiLU backward case (tests/test_hip_backward.py test_gn_film_silu_backward)."""
    B, Ca, Cb, Hs, Ws, rs, act, use_film, add_mode, accumulate = case[:10]
    tag = "t/bwd/gn/" + "_".join(map(str, case))
    C = Ca + Cb
    Hc, Wc = (Hs * 2, Ws * 2) if rs == 1 else ((Hs // 2, Ws // 2) if rs == 2 else (Hs, Ws))
    t = dict(xa=fx.randn(tag + "/xa", B, Ca, Hs, Ws) * 1.3 + 0.4, xb=fx.randn(tag + "/xb", B, Cb, Hs, Ws) * 0.7 if Cb else None,
             gamma=fx.param(tag, "norm.weight", (C,)), beta=fx.param(tag, "norm.bias", (C,)),
             film=fx.randn(tag + "/film", B, 2 * C) * 0.3 if use_film else None, dact=fx.randn(tag + "/dact", B, C, Hc, Wc), add=None)
    if add_mode == 1:
        t["add"] = fx.randn(tag + "/add", B, C, Hs, Ws)
    elif add_mode == 2:
        t["add"] = fx.randn(tag + "/add", B, C, Hc, Wc)
    t["init"] = (fx.randn(tag + "/ia", B, Ca, Hs, Ws), fx.randn(tag + "/ib", B, Cb, Hs, Ws) if Cb else None) if accumulate else None
    return t


GN_OUT = ("dxa", "dxb", "dgamma", "dbeta", "dfilm")


def gn_reference(case, t, dtype=torch.float32):
    """{dxa, dxb, dgamma, dbeta, dfilm} (None where the case has none) by autograd through the oracle in ``dtype``.  float32 is what
    test_gn_film_silu_backward has always compared with; the knob tests take float64."""
    B, Ca, Cb, Hs, Ws, rs, act, use_film, add_mode, accumulate = case[:10]
    C = Ca + Cb
    c = lambda v: None if v is None else v.to(dtype)  # noqa: E731
    xa, gamma, beta = (c(t[k]).requires_grad_(True) for k in ("xa", "gamma", "beta"))
    xb = c(t["xb"]).requires_grad_(True) if Cb else None
    film = c(t["film"]).requires_grad_(True) if use_film else None
    x = torch.cat([xa, xb], 1) if Cb else xa
    y = orc.group_norm(x, gamma, beta)
    if use_film:
        y = torch.addcmul(film[:, C:, None, None], y, film[:, :C, None, None] + 1)
    u = F.silu(y) if act else y
    res = orc.resample_up if rs == 1 else (orc.resample_down if rs == 2 else (lambda v: v))
    loss = (res(u) * c(t["dact"])).sum()
    if add_mode == 1:
        loss = loss + (x * c(t["add"])).sum()
    elif add_mode == 2:
        loss = loss + (res(x) * c(t["add"])).sum()
    ins = [xa, gamma, beta] + ([xb] if Cb else []) + ([film] if use_film else [])
    gr = torch.autograd.grad(loss, ins)
    out = dict(dxa=gr[0], dgamma=gr[1], dbeta=gr[2], dxb=gr[3] if Cb else None, dfilm=gr[-1] if use_film else None)
    if accumulate:
        out["dxa"] = out["dxa"] + c(t["init"][0])
        if Cb:
            out["dxb"] = out["dxb"] + c(t["init"][1])
    return out


@functools.lru_cache(maxsize=None)
def gn_reference64(case):
    return gn_reference(case, gn_inputs(case), torch.float64)


@functools.lru_cache(maxsize=None)
def c1_reference64(shape):
    return c1_reference(c1_inputs(shape))


# ---------------------------------------------------------------------------------------------------------------------------------
# device runs (child and parent alike)


def dev(t):
    return None if t is None else t.detach().contiguous().cuda()


def row_tokens(report):
    """The rows of a profiler report as names: "name", or "name[variant]" once per variant where the launches of a row named the
    kernel or instantiation they took (csrc/prof.hpp ProfScope: launch_attention, try_launch_conv1x1_reg, the two-pass
    gn_bwd_kernel)."""
    out = set()
    for r in report:
        out |= {f"{r['name']}[{v}]" for v in r["variants"]} if r.get("variants") else {r["name"]}
    return sorted(out)


def profiled(L, fn):
    """fn() with the profiler on -> (its result, row_tokens of the rows it left)."""
    torch.cuda.synchronize()
    L.prof_enable(True)
    try:
        out = fn()
        torch.cuda.synchronize()
        rows = row_tokens(L.prof_report())
    finally:
        L.prof_enable(False)
    return out, rows


def run_gn(L, case, t):
    """-> ({dxa, dxb, dgamma, dbeta, dfilm}, profiler rows, sum of |sync| afterwards or None)."""
    B, Ca, Cb, Hs, Ws, rs, act, use_film, add_mode, accumulate = case[:10]
    C = Ca + Cb
    xa, xb, gamma, beta, film = (dev(t[k]) for k in ("xa", "xb", "gamma", "beta", "film"))
    coef, stats = L.op_gn_coef(xa, xb, gamma, beta, film=film, film_batch=1, film_stride=2 * C, want_stats=True)
    sync = torch.zeros(L.GN_SYNC_WORDS * B * gn_groups(C), dtype=torch.int32, device="cuda") if len(case) > 10 else None
    init = (dev(t["init"][0]), dev(t["init"][1])) if accumulate else None
    got, rows = profiled(L, lambda: L.op_gn_bwd(dev(t["dact"]), xa, xb, coef, stats, gamma, beta, film=film, film_batch=1,
                                                film_stride=2 * C, act=act, resample=rs, add=dev(t["add"]), add_mode=add_mode,
                                                dx_init=init, sync=sync))
    return dict(zip(GN_OUT, got)), rows, None if sync is None else int(sync.abs().sum())


def run_c1(L, shape, t, reg=1):
    """op_conv with the register-direct kernel forced on (reg = 1) or off (0) -> (out, profiler rows, (wpk, bpk))."""
    wpk, bpk = L.op_pack_conv(dev(t["w"]), dev(t["b"]))
    L.set_conv1x1_reg(reg)
    try:
        out, rows = profiled(L, lambda: L.op_conv(dev(t["xa"]), dev(t["xb"]), wpk, bpk, shape[3], 1,
                                                  **(dict(res=dev(t["res"])) if t["res"] is not None else {})))
    finally:
        L.set_conv1x1_reg(-1)
    return out, rows, (wpk, bpk)


def run_attn(L, shape, kind, pair):
    """-> (a, dqkv or None, profiler rows), both in the kernels' packed layout."""
    case = attn_case(shape)
    qkv, da = AB.inputs(case, kind)
    pq = dev(AB.packed_qkv(qkv, case.heads))
    assert pq.data_ptr() % 16 == 0

    def go():
        a = L.op_attention(pq, case.heads)
        if not pair:
            return a, None
        out = torch.full(pq.shape, float("nan"), device="cuda")
        return a, L.op_attention_bwd(pq, a, dev(da), case.heads, out=out)
    (a, g), rows = profiled(L, go)
    return a, g, rows


def run_case(L, key):
    """-> {key + "/" + name: array}; the profiler rows as one ";"-joined string under key + "/rows"."""
    c = CASES[key]
    r = {}
    if c.kind in ("attn_fwd", "attn_pair"):
        a, g, rows = run_attn(L, c.shape, c.sub, c.kind == "attn_pair")
        r["a"] = a
        if g is not None:
            r["dqkv"] = g
    elif c.kind == "c1":
        r["out"], rows, _ = run_c1(L, c.shape, c1_inputs(c.shape))
    elif c.kind == "wino":
        r["out"], rows = run_wino(L, c.shape, wino_inputs(c.shape))
    else:
        assert c.kind == "gn", c.kind
        got, rows, left = run_gn(L, c.shape, gn_inputs(c.shape))
        r.update({k: v for k, v in got.items() if v is not None})
        if left is not None:
            r["sync_left"] = torch.tensor(left)
    out = {f"{key}/{k}": v.detach().cpu().numpy() for k, v in r.items()}
    out[key + "/rows"] = np.array(";".join(rows))
    return out


def run_group(L, name):
    out = {}
    for key in GROUPS[name][1]:
        out.update(run_case(L, key))
    return out


def rows_ok(case, rows):
    """rows: the list of profiler rows a case left -> the list of complaints (empty: as the table says)."""
    hit = lambda pat, r: r.startswith(pat[:-1]) if pat.endswith("*") else r == pat  # noqa: E731
    bad = [f"missing {m}" for m in case.must if not any(hit(m, r) for r in rows)]
    for n in case.must_not:
        bad += [f"forbidden {r}" for r in rows if (r.startswith(n[:-1]) if n.endswith("*") else r == n)]
    return bad


if __name__ == "__main__":
    lib = importlib.import_module("m-cedm_amd.lib")
    lib.load()
    np.savez(sys.argv[2], **run_group(lib, sys.argv[1]))
