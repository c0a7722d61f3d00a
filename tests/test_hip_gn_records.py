"""The fused GroupNorm statistics chain at kernel level, against fp64 (tests/_gn_records.py).

Inference in both U-Nets runs no GroupNorm kernel: every conv that produces a normalised tensor writes per-tile (sum, M2) records
in its epilogue, and the next conv merges them in fp64 -- inside the kernel (conv_tile.hpp stage_coef_rows, gn_on) or in
gn_coef_from_sums_kernel (training layout).  Here every record WRITER is compared with the fp64 records of its own output, per
record (a record under the wrong tile index, an M2 about the wrong mean, a dropped row or a crossed channel pair each fail), and
both READERS with the fp64 GroupNorm, on inputs whose mean is 20+ standard deviations (bias of the producing conv +-30, spread ~1):
E[x^2] - E[x]^2 arithmetic in fp32 and a wrong-mean M2 both show there.

Bars: outputs at the file-wide bar of test_hip_parity.py (rtol 1e-4, atol 1e-5); group statistics and normalised tensors at the bar
of test_gn_coef_golden (the same numbers); records at the analytic bounds derived in tests/_gn_records.py.
Run with -s for the largest observed err / bound per kernel family."""
import math
from contextlib import contextmanager

import pytest
import torch
import torch.nn.functional as F

from oracle import fixtures as fx
from tests import _gn_records as R
from tests import _wino_fold as WF

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-4, 1e-5
EPS = 1e-5
WORST = {}                       # kernel family -> [largest err / bound of a record (d), of a group statistic or an output (e)]
REFS = {}                        # tag -> (inputs, fp64 reference): computed once, shared, never modified


@pytest.fixture(scope="module")
def lib():
    import mcedm_amd  # noqa: F401
    from mcedm_amd import lib as L
    assert torch.cuda.is_available(), "these tests need the MI355X"
    L.load()
    return L


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    for fam, (d, e) in sorted(WORST.items()):
        if d:          # a record writer: checks (d) and (e)
            print(f"\n[gn-records] {fam}: largest err / bound: records {d:.3e}, merged group statistics {e:.3e}", end="")
        else:          # a reader, or the chain
            print(f"\n[gn-records] {fam}: largest err / bound: {e:.3e}", end="")
    print()


def note(family, d=0.0, e=0.0):
    w = WORST.setdefault(family, [0.0, 0.0])
    w[0], w[1] = max(w[0], d), max(w[1], e)


def dev(t):
    return None if t is None else t.cuda().contiguous()


def close(got, ref, what=""):
    got, ref = got.detach().cpu().double(), torch.as_tensor(ref).double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = (got - ref).abs()
    bad = ~(err <= ATOL + RTOL * ref.abs())
    assert not bad.any(), f"{what}: {int(bad.sum())}/{bad.numel()} out of tolerance, max err {err.max():.3e} (max ref {ref.abs().max():.3e})"
    return float((err / (ATOL + RTOL * ref.abs())).max())


@contextmanager
def overrides(lib, tile=None, resident=None, wino1=None):
    """Kernel selection as in the existing tests; every override is restored whatever happens."""
    try:
        if tile:
            lib.set_conv_tile(*tile)
        if resident is not None:
            lib.set_conv_resident(resident)
        if wino1 is not None:
            lib.set_conv_wino1(wino1)
        yield
    finally:
        lib.set_conv_tile()
        lib.set_conv_resident(-1)
        lib.set_conv_wino1(-1)


def profiled(lib, fn):
    lib.prof_enable(True)
    try:
        out = fn()
        torch.cuda.synchronize()
        names = [r["name"] for r in lib.prof_report()]
    finally:
        lib.prof_enable(False)
    return out, names


def ran(names, kernel, what):
    assert any(n.startswith(kernel) for n in names), f"{what}: expected {kernel}, ran {names}"


def apply_coef(x, coef, act=False):
    y = (x - coef[:, :, 0, None, None]) * coef[:, :, 1, None, None] + coef[:, :, 2, None, None]
    return F.silu(y) if act else y


def up2(x):
    return x.repeat_interleave(2, 2).repeat_interleave(2, 3)


def groups_for(C, rc):
    """GroupNorm(32) of the DDPM U-Net where pair records serve it (2-channel groups at C = 64), min(32, C / 4) of the ADM U-Net."""
    if rc == 2:
        return 32 if C % 32 == 0 else C // 2
    g = min(32, C // 4)
    return g if (C // g) % 4 == 0 else C // 4          # C = 192: 6-channel groups are no whole quads (such a norm takes gn_coef_kernel)


# ------------------------------------------------------------------------------------------------ producers
def conv_case(tag, B, Ca, Cb, Cout, H, W, k, rs=0, rm=None, transform=True, sign=1.0, bias_rows=False):
    """Inputs and fp64 reference of out = conv_k(resample(silu(coef(cat(xa, xb))))) + bias + resample(res), bias = +-30."""
    if tag in REFS:
        return REFS[tag]
    Cin = Ca + Cb
    Hs, Ws = {0: (H, W), 1: (H // 2, W // 2), 2: (2 * H, 2 * W), 3: (2 * H, 2 * W)}[rs]
    t = dict(B=B, Ca=Ca, Cb=Cb, Cout=Cout, H=H, W=W, k=k, rs=rs, rm=rm, transform=transform, bias_rows=bias_rows)
    t["xa"] = fx.randn(tag + "/xa", B, Ca, Hs, Ws)
    t["xb"] = fx.randn(tag + "/xb", B, Cb, Hs, Ws) if Cb else None
    # (a spread of about 1 in every GroupNorm group of the output: SiLU of the transformed input has an rms of about 0.6 and a mean
    # that the weights turn into an offset per channel; residual and bias add theirs)
    t["w"] = fx.randn(tag + "/w", Cout, Cin, k, k) * ((1.25 if transform else 0.85) / math.sqrt(Cin * k * k))
    t["b"] = sign * 30.0 + 0.2 * (fx.randn(tag + "/b", B, Cout) if bias_rows else fx.randn(tag + "/b", Cout))
    t["coef"] = torch.stack([fx.randn(tag + "/mean", B, Cin) * 0.3, 1 + 0.3 * fx.randn(tag + "/scale", B, Cin),
                             0.2 * fx.randn(tag + "/off", B, Cin), torch.zeros(B, Cin)], dim=-1) if transform else None
    Hr, Wr = {None: (0, 0), 0: (H, W), 1: (H // 2, W // 2), 2: (2 * H, 2 * W)}[rm]
    t["res"] = 0.35 * fx.randn(tag + "/res", B, Cout, Hr, Wr) if rm is not None else None
    x = (torch.cat([t["xa"], t["xb"]], 1) if Cb else t["xa"]).double()
    if transform:
        x = apply_coef(x, t["coef"].double(), True)
    x = up2(x) if rs == 1 else (F.avg_pool2d(x, 2) if rs == 2 else x)
    if rs == 3:
        ref = F.conv2d(F.pad(x, (0, 1, 0, 1)), t["w"].double(), stride=2)
    else:
        ref = F.conv2d(x, t["w"].double(), padding=k // 2)
    ref = ref + (t["b"].double()[:, :, None, None] if bias_rows else t["b"].double()[None, :, None, None])
    if rm is not None:
        r = t["res"].double()
        ref = ref + (up2(r) if rm == 1 else (F.avg_pool2d(r, 2) if rm == 2 else r))
    REFS[tag] = (t, ref)
    return REFS[tag]


def run_conv_case(lib, t, rc, wino=False):
    """-> (out, records, tiling, kernel names, the same launch without gsum)."""
    B, Cout, k = t["B"], t["Cout"], t["k"]
    xa, xb = dev(t["xa"]), dev(t["xb"])
    wpk, bpk = lib.op_pack_conv(dev(t["w"]), None if t["bias_rows"] else dev(t["b"]))
    bias, pitch = (dev(t["b"]), Cout) if t["bias_rows"] else (bpk, 0)
    table = lib.op_pack_conv_wino(dev(t["w"])) if wino else None
    kw = dict(coef=dev(t["coef"]), act=int(t["transform"]), resample=t["rs"], res=dev(t["res"]), res_mode=t["rm"] or 0)
    (out, rec, tiling), names = profiled(lib, lambda: lib.op_conv_sums(xa, xb, wpk, bias, Cout, k, rc=rc, wino=table, bias_batch=pitch, **kw))
    if not wino:
        plain = lib.op_conv(xa, xb, wpk, bias, Cout, k, bias_batch=pitch, **kw)
    elif t["bias_rows"]:      # sample b of the per-sample form == the single-row entry on sample b with row b (include/mcedm_hip.h)
        plain = torch.cat([lib.op_conv_wino(xa[i:i + 1], None, table, dev(t["b"][i]), Cout, coef=dev(t["coef"][i:i + 1]), act=1,
                                            res=None if t["res"] is None else dev(t["res"][i:i + 1])) for i in range(B)])
    else:
        plain = lib.op_conv_wino(xa, xb, table, bpk, Cout, **kw)
    return out, rec, tiling, names, plain


def check_producer(family, what, t, ref, out, rec, tiling, plain, rc, tile=None):
    """(a) - (e) of the producers."""
    B, Cout, H, W = t["B"], t["Cout"], t["H"], t["W"]
    assert tuple(tiling)[4] == rc, (what, tiling)
    if tile:
        tx = -(-W // tile[1])
        assert tuple(tiling) == (tx * -(-H // tile[0]), tx, tile[0], tile[1], rc), (what, tiling)
    assert torch.equal(out, plain), f"{what}: (a) asking for records changed {int((out != plain).sum())} of {out.numel()} outputs"
    close(out, ref, what + ": (b) output vs fp64")
    assert tuple(rec.shape) == (B, tiling[0], Cout // rc, 2), (what, tuple(rec.shape), tiling)
    assert not torch.isnan(rec).any(), f"{what}: (c) {int(torch.isnan(rec).any(-1).sum())} of {rec[..., 0].numel()} records were never written"
    d = R.check_records(rec, out, tiling, what + ": (d)")
    groups = groups_for(Cout, rc)
    gm, gr = R.group_stats64(ref, groups, EPS)
    ratio = float((gm.abs() * gr).min())
    assert ratio > 20, f"{what}: |mean| / std = {ratio:.1f} on the fp64 reference"
    e = R.check_groups(*R.merge64(rec, tiling, H, W, groups, Cout, eps=EPS), gm, gr, what=what + ": (e)")
    print(f"{what}: tiling {tuple(tiling)}, |mean|/std {ratio:.0f}, err / bound: records {d:.3e}, groups {e:.3e}")
    note(family, d, e)


TILES = [(128, 8, 32), (64, 8, 32), (32, 8, 32), (128, 16, 16), (64, 16, 16), (32, 16, 16), (128, 8, 16), (64, 8, 16),
         (128, 8, 8), (64, 8, 8), (32, 8, 8), (128, 16, 32)]       # = TILES of test_hip_parity.py
MFMA_CASES = [(tile, k, rc) for tile in TILES for k in (3, 1) for rc in (4, 2)
              if not (tile == (128, 16, 32) and (k == 1 or rc == 2))]      # the 8-wave kernel: 3x3, quad records only


@pytest.mark.parametrize("tile,k,rc", MFMA_CASES)
def test_conv_mfma_records_every_tile(lib, tile, k, rc):
    """Every instantiation of conv_mfma_kernel (and the 8-wave kernel's two-sub-tile store) on the ragged problem of
    test_conv_every_tile_configuration: 72|64 -> 128 channels at 40 x 24, with transform rows, SiLU and a residual.  On
    (128, 16, 32) the 40 rows leave the last 16-row tile with one live 8-row sub-tile."""
    t, ref = conv_case(f"gnrec/tiles/k{k}", 2, 72, 64, 128, 40, 24, k, rm=0)
    with overrides(lib, tile=tile):
        out, rec, tiling, names, plain = run_conv_case(lib, t, rc)
    what = f"tile {tile} k={k} rc={rc}"
    if tile == (128, 16, 32):
        ran(names, "conv8_mfma_kernel<ConvCfg<128, 16, 32,", what)
        check_producer("conv8_mfma_kernel", what, t, ref, out, rec, tiling, plain, rc, tile=(8, 32))
    else:
        ran(names, f"conv_mfma_kernel<ConvCfg<{tile[0]}, {tile[1]}, {tile[2]},", what)
        check_producer("conv_mfma_kernel", what, t, ref, out, rec, tiling, plain, rc, tile=tile[1:])


@pytest.mark.parametrize("rc", [4, 2])
@pytest.mark.parametrize("resident,B,H,W", [(0, 3, 8, 8), (0, 2, 20, 12), (1, 3, 8, 8)])
def test_records_of_a_partial_channel_tile(lib, resident, B, H, W, rc):
    """Cout = 72 pads to 96 and the last 32-channel tile has 8 live rows (FULL == false): conv_mfma_kernel<32, 8, 8>, and the tiles
    of 32 channels that conv_resident_kernel uses on <= 8 x 8 images (the only ones it has)."""
    t, ref = conv_case(f"gnrec/partial/{B}_{H}_{W}", B, 40, 0, 72, H, W, 3, rm=0, sign=-1.0)
    what = f"partial channel tile {H} x {W} rc={rc} resident={resident}"
    with overrides(lib, tile=None if resident else (32, 8, 8), resident=resident):
        out, rec, tiling, names, plain = run_conv_case(lib, t, rc)
    if resident:
        ran(names, "conv_resident_kernel<ResCfg<32, 4, 8,", what)
        check_producer("conv_resident_kernel", what, t, ref, out, rec, tiling, plain, rc, tile=(4, 8))
    else:
        ran(names, "conv_mfma_kernel<ConvCfg<32, 8, 8,", what)
        check_producer("conv_mfma_kernel", what, t, ref, out, rec, tiling, plain, rc, tile=(8, 8))


RESAMPLED = {
    # name: (conv_case arguments, kernel the profiler must name)
    "up": (dict(B=2, Ca=64, Cb=0, Cout=64, H=16, W=16, k=3, rs=1, rm=0), "conv_mfma_kernel<ConvCfg<64, 8, 8,"),
    "down": (dict(B=2, Ca=64, Cb=0, Cout=64, H=16, W=16, k=3, rs=2, rm=0), "conv_mfma_kernel<ConvCfg<64, 8, 8,"),
    "s2_ragged": (dict(B=2, Ca=40, Cb=0, Cout=24, H=10, W=6, k=3, rs=3), "conv_s2_mfma_kernel<ConvCfg<32, 8, 8,"),
    "s2_64": (dict(B=3, Ca=64, Cb=0, Cout=64, H=8, W=8, k=3, rs=3, transform=False), "conv_s2_mfma_kernel<ConvCfg<64, 8, 8,"),
    "res_half": (dict(B=2, Ca=64, Cb=0, Cout=64, H=16, W=16, k=3, rm=1), "conv_mfma_kernel<ConvCfg<64, 8, 8,"),
    "res_double": (dict(B=2, Ca=64, Cb=0, Cout=64, H=16, W=16, k=3, rm=2), "conv_mfma_kernel<ConvCfg<64, 8, 8,"),
}


@pytest.mark.parametrize("rc", [4, 2])
@pytest.mark.parametrize("name", list(RESAMPLED))
def test_records_of_resampling_convs(lib, name, rc):
    """conv_mfma_kernel's RS_UP and RS_DOWN forms, conv_s2_mfma_kernel on the two smallest shapes of
    test_conv_stride2_ddpm_downsample, and a residual at half and at double resolution."""
    args, kernel = RESAMPLED[name]
    t, ref = conv_case("gnrec/rs/" + name, **args)
    with overrides(lib, resident=0):
        out, rec, tiling, names, plain = run_conv_case(lib, t, rc)
    what = f"{name} rc={rc}"
    ran(names, kernel, what)
    if name in ("up", "down"):
        assert any(n.endswith(f", {args['rs']}>") for n in names if n.startswith(kernel)), (what, names)
    check_producer(kernel.split("<")[0], what, t, ref, out, rec, tiling, plain, rc, tile=(8, 8))


RESIDENT = {
    # (B, Ca, Cb, Cout, H, W, k) from test_conv_resident_kernel_is_bit_identical_to_the_tiled_one: (kernel, its pixel tile)
    (3, 64, 0, 64, 8, 8, 3): ("conv_resident_kernel<ResCfg<32, 4, 8, 1, 1, 9, 8, 4>", (4, 8)),         # the K-split tile
    (2, 64, 0, 64, 16, 16, 3): ("conv_resident_kernel<ResCfg<64, 8, 8, 2, 2, 9, 8,", (8, 8)),
    (2, 64, 0, 64, 32, 32, 3): ("conv_resident_kernel<ResCfg<64, 8, 16, 1, 4, 9, 8,", (8, 16)),
    (2, 24, 12, 64, 12, 10, 3): ("conv_resident_kernel<ResCfg<64, 8, 8, 2, 2, 9, 8,", (8, 8)),          # ragged both ways
    (1, 72, 0, 64, 28, 30, 3): ("conv_resident_kernel<ResCfg<64, 8, 16, 1, 4, 9, 8,", (8, 16)),         # ragged both ways
    (2, 64, 0, 64, 64, 64, 3): ("conv_resident_kernel<ResCfg<64, 8, 32, 1, 4, 9, 8,", (8, 32)),         # the big tile
    (2, 64, 0, 192, 8, 8, 1): ("conv_resident_kernel<ResCfg<64, 8, 8, 2, 2, 1, 16,", (8, 8)),
}


@pytest.mark.parametrize("shape,rc", [(s, rc) for s in RESIDENT for rc in (4, 2) if rc == 4 or s[3] == 64])
def test_conv_resident_records(lib, shape, rc):
    B, Ca, Cb, Cout, H, W, k = shape
    kernel, tile = RESIDENT[shape]
    t, ref = conv_case("gnrec/resident/" + "_".join(map(str, shape)), B, Ca, Cb, Cout, H, W, k, rm=0)
    with overrides(lib, resident=1):
        out, rec, tiling, names, plain = run_conv_case(lib, t, rc)
    what = f"resident {shape} rc={rc}"
    ran(names, kernel, what)
    check_producer("conv_resident_kernel", what, t, ref, out, rec, tiling, plain, rc, tile=tile)


WINO = {
    # through the dispatcher (>= 32 x 32: it prefers the Winograd kernels there), pair and quad records
    "128_32x32": (dict(B=2, Ca=128, Cb=0, Cout=128, H=32, W=32, k=3, rm=0), "conv_wino_kernel<WinoCfg<4>, false, true>"),
    "64_32x32": (dict(B=2, Ca=64, Cb=0, Cout=64, H=32, W=32, k=3, rm=0), "conv_wino_kernel<WinoCfg<2>, false, true>"),
    "up_32x32": (dict(B=2, Ca=64, Cb=0, Cout=64, H=32, W=32, k=3, rs=1), "conv_wino_kernel<WinoCfg<2>, true, true"),
    "bias_rows": (dict(B=3, Ca=64, Cb=0, Cout=64, H=32, W=32, k=3, bias_rows=True), "conv_wino_kernel<WinoCfg<2>, false, true, WinoBiasRows>"),
}


@pytest.mark.parametrize("rc", [4, 2])
@pytest.mark.parametrize("name", list(WINO))
def test_conv_wino_records(lib, name, rc):
    args, kernel = WINO[name]
    t, ref = conv_case("gnrec/wino/" + name, sign=-1.0, **args)
    with overrides(lib, wino1=0):
        out, rec, tiling, names, plain = run_conv_case(lib, t, rc, wino=True)
    what = f"wino {name} rc={rc}"
    ran(names, kernel, what)
    check_producer("conv_wino_kernel", what, t, ref, out, rec, tiling, plain, rc, tile=(8, 16))


@pytest.mark.parametrize("rc", [4, 2])
@pytest.mark.parametrize("name", ["128_32x32", "up128"])
def test_conv_wino1_records(lib, name, rc):
    """The one-wave-per-SIMD kernel that serves the 128-channel shapes when switched on."""
    args = WINO["128_32x32"][0] if name == "128_32x32" else dict(B=2, Ca=128, Cb=0, Cout=128, H=32, W=32, k=3, rs=1)
    t, ref = conv_case("gnrec/wino/" + name, sign=-1.0, **args)
    with overrides(lib, wino1=1):
        out, rec, tiling, names, plain = run_conv_case(lib, t, rc, wino=True)
    what = f"wino1 {name} rc={rc}"
    ran(names, "conv_wino1_kernel<true>" if args.get("rs") else "conv_wino1_kernel<false>", what)
    check_producer("conv_wino1_kernel", what, t, ref, out, rec, tiling, plain, rc, tile=(8, 16))


@pytest.mark.parametrize("B,C,H,W", [(2, 64, 8, 16), (2, 64, 16, 32)])
def test_conv_wino_records_below_the_dispatchers_size(lib, B, C, H, W):
    """One tile, and 2 x 2 tiles: images the dispatcher does not give to the Winograd kernel, through mcedm_op_conv_wino_sums (quad
    records; the tiling is the kernel's fixed 8 x 16)."""
    t, ref = conv_case(f"gnrec/wino/small{H}x{W}", B, C, 0, C, H, W, 3, rm=0)
    table = lib.op_pack_conv_wino(dev(t["w"]))
    kw = dict(coef=dev(t["coef"]), act=1, res=dev(t["res"]))
    (out, gsum), names = profiled(lib, lambda: lib.op_conv_wino(dev(t["xa"]), None, table, dev(t["b"]), C, want_sums=True, **kw))
    plain = lib.op_conv_wino(dev(t["xa"]), None, table, dev(t["b"]), C, **kw)
    tiling = ((H // 8) * (W // 16), W // 16, 8, 16, 4)
    rec = gsum[:B * tiling[0] * (C // 4) * 2].view(B, tiling[0], C // 4, 2)
    what = f"wino {C} channels at {H} x {W}"
    ran(names, "conv_wino_kernel<WinoCfg<2>, false, true>", what)
    check_producer("conv_wino_kernel", what, t, ref, out, rec, tiling, plain, 4)


def test_conv_wino_skip_records(lib):
    """The SKIP form (the folded 1x1 projection computed in the epilogue), case b2_128_128 of tests/_wino_fold.py through the
    existing mcedm_op_conv_skip, with a large-mean bias."""
    name = "b2_128_128"
    B, Ca, Cb, Cout, H, W = WF.CASES[name]
    if "gnrec/skip" not in REFS:
        t = dict(WF.case_inputs(name))
        t["b"] = 30.0 + 0.3 * fx.randn("gnrec/skip/b", Cout)
        REFS["gnrec/skip"] = (t, WF.case_reference(t))
    t, ref = REFS["gnrec/skip"]
    wpk, bpk = lib.op_pack_conv(dev(t["w"]), dev(t["b"]))
    spk, sbias = lib.op_pack_conv(dev(t["ws"]), dev(t["bs"]))
    args = (dev(t["h"]), wpk, lib.op_pack_conv_wino(dev(t["w"])), bpk, Cout)
    kw = dict(coef=dev(t["coef"]), sk_xa=dev(t["xa"]), sk_xb=dev(t["xb"]), sk_wpk=spk, sk_wfrag=lib.op_pack_conv_frag(dev(t["ws"])), sk_bias=sbias)
    (out, gsum), names = profiled(lib, lambda: lib.op_conv_skip(*args, want_sums=True, **kw))
    plain = lib.op_conv_skip(*args, **kw)
    ran(names, "conv_wino_kernel<WinoSkipCfg<4>, false, true>", name)
    tiling = ((H // 8) * (W // 16), W // 16, 8, 16, 4)
    rec = gsum[:B * tiling[0] * (Cout // 4) * 2].view(B, tiling[0], Cout // 4, 2)
    check_producer("conv_wino_kernel", "wino SKIP " + name, dict(B=B, Cout=Cout, H=H, W=W), ref, out, rec, tiling, plain, 4)


@pytest.mark.parametrize("rc", [2, 4])
@pytest.mark.parametrize("C", [64, 128])
def test_records_of_the_attention_projection(lib, C, rc):
    """The 1x1 projection with residual that the DDPM attention block launches (ddpm.hip attn_block): no transform, no activation."""
    t, ref = conv_case(f"gnrec/proj/{C}", 2, C, 0, C, 16, 16, 1, rm=0, transform=False)
    out, rec, tiling, names, plain = run_conv_case(lib, t, rc)
    what = f"attention projection {C} rc={rc}"
    ran(names, "conv_resident_kernel<ResCfg<64, 8, 8, 2, 2, 1, 16,", what)
    check_producer("conv_resident_kernel", what, t, ref, out, rec, tiling, plain, rc, tile=(8, 8))


# ------------------------------------------------------------------------------------------------ consumers
# name: B, H, W, groups, FiLM (None / "batch" / "bcast"), parts = [(channels, (mt, ph, pw) of the producing tile, rc)]; real: a
# conv_mfma_kernel launch with that forced tile can produce the records (else synthetic records only)
SETS = {
    "pairs64": dict(B=2, H=16, W=16, groups=32, film=None, parts=[(64, (64, 8, 8), 2)], real=True),
    "quads128": dict(B=2, H=40, W=24, groups=32, film="batch", parts=[(128, (128, 8, 32), 4)], real=True),
    "quads256": dict(B=3, H=16, W=16, groups=32, film="bcast", parts=[(256, (128, 8, 8), 4)], real=True),
    "tiles180": dict(B=2, H=80, W=72, groups=4, film=None, parts=[(16, (0, 4, 8), 4)], real=False),        # 180 tiles > 64 lanes, ragged
    "cat64p_192q": dict(B=3, H=24, W=24, groups=32, film="batch", parts=[(64, (64, 8, 8), 2), (192, (64, 8, 16), 4)], real=True),
    "cat132_124": dict(B=2, H=40, W=24, groups=32, film="bcast", parts=[(132, (32, 8, 32), 4), (124, (64, 16, 16), 4)], real=True),
    "adm64": dict(B=2, H=16, W=16, groups=16, film=None, parts=[(64, (64, 8, 8), 4)], real=True),           # min(32, C / 4)
    "wino128": dict(B=2, H=32, W=32, groups=32, film="batch", parts=[(128, (128, 8, 16), 4)], real=True),
    "pairs64_64x64": dict(B=2, H=64, W=64, groups=32, film=None, parts=[(64, (0, 4, 8), 2)], real=False),   # 128 tiles
    "c8g2": dict(B=2, H=80, W=72, groups=2, film=None, parts=[(8, (0, 4, 8), 4)], real=False),              # lanes per group cap at 64
}
SET_CACHE = {}


def record_set(lib, name, source):
    """-> dict(x parts (CPU fp32), records, tilings, gamma, beta, film rows, fp64 GroupNorm (+ FiLM) of the tensor, fp64 stats)."""
    key = (name, source)
    if key in SET_CACHE:
        return SET_CACHE[key]
    s = SETS[name]
    B, H, W = s["B"], s["H"], s["W"]
    xs, recs, tilings = [], [], []
    for i, (C, tile, rc) in enumerate(s["parts"]):
        tag = f"gnrec/set/{name}/{i}"
        sign = -1.0 if i else 1.0
        if source == "real":
            t, _ = conv_case(tag, B, 16, 0, C, H, W, 3, sign=sign)
            with overrides(lib, tile=tile):
                out, rec, tiling, names, _ = run_conv_case(lib, t, rc)
            ran(names, f"conv_mfma_kernel<ConvCfg<{tile[0]}, {tile[1]}, {tile[2]},", tag)
            xs.append(out.cpu())
            recs.append(rec)
            tilings.append(tuple(tiling))
        else:
            x = fx.randn(tag + "/x", B, C, H, W) + sign * 30.0 + 0.3 * fx.randn(tag + "/m", C)[None, :, None, None]
            tx = -(-W // tile[2])
            tiling = (tx * -(-H // tile[1]), tx, tile[1], tile[2], rc)
            xs.append(x)
            recs.append(dev(R.synthetic_records(x, tiling)))
            tilings.append(tiling)
    C = sum(p[0] for p in s["parts"])
    gamma, beta = 1 + 0.2 * fx.randn(f"gnrec/set/{name}/g", C), 0.2 * fx.randn(f"gnrec/set/{name}/b", C)
    x64 = torch.cat(xs, 1).double()
    ref = F.group_norm(x64, s["groups"], gamma.double(), beta.double(), EPS)
    film = None
    if s["film"]:
        rows, stride = (B if s["film"] == "batch" else 1), 2 * C + 24
        film = 0.3 * fx.randn(f"gnrec/set/{name}/film", rows, stride)
        sc, sh = film[:, 8:8 + C, None, None].double(), film[:, 8 + C:8 + 2 * C, None, None].double()
        ref = torch.addcmul(sh, ref, sc + 1)
    gm, gr = R.group_stats64(x64, s["groups"], EPS)
    if len(s["parts"]) == 1:          # (the two sources of a concat have means of opposite sign)
        assert float((gm.abs() * gr).min()) > 20, (name, source)
    SET_CACHE[key] = dict(xs=xs, recs=recs, tilings=tilings, gamma=gamma, beta=beta, film=film, ref=ref, gm=gm, gr=gr, C=C)
    return SET_CACHE[key]


def gn_kwargs(s, r):
    kw = dict(film=None if r["film"] is None else dev(r["film"][:, 8:]), film_batch=int(s["film"] == "batch"),
              film_stride=0 if r["film"] is None else r["film"].shape[1] - 8, eps=EPS)
    if len(r["recs"]) > 1:
        kw.update(sumb=r["recs"][1], tiling_b=r["tilings"][1])
    return kw


def coef_table(lib, name, r):
    s = SETS[name]
    Ca = s["parts"][0][0]
    return lib.op_gn_coef_from_sums(r["recs"][0], r["tilings"][0], Ca, s["H"], s["W"], s["groups"], dev(r["gamma"]), dev(r["beta"]),
                                    Cb=r["C"] - Ca, **gn_kwargs(s, r))


SET_SOURCES = [(n, src) for n in SETS for src in ("synthetic", "real") if src == "synthetic" or SETS[n]["real"]]


@pytest.mark.parametrize("name,source", SET_SOURCES)
def test_gn_coef_from_sums_kernel(lib, name, source):
    """The table kernel of the training layout on records alone: its rows applied as apply_coef does against the fp64 GroupNorm
    (+ FiLM per sample / broadcast) of the tensor the records describe, its statistics against the fp64 mean / rstd."""
    s, r = SETS[name], record_set(lib, name, source)
    (coef, stats), names = profiled(lib, lambda: coef_table(lib, name, r))
    what = f"gn_coef_from_sums {name} ({source} records)"
    assert names == ["gn_coef_from_sums_kernel"], (what, names)
    assert tuple(coef.shape) == (s["B"], r["C"], 4) and tuple(stats.shape) == (s["B"], s["groups"], 2)
    x = torch.cat(r["xs"], 1)
    close(apply_coef(x.double(), coef.cpu().double()), r["ref"], what + ": normalised tensor")
    e = R.check_groups(stats[..., 0], stats[..., 1], r["gm"], r["gr"], what=what)
    note("gn_coef_from_sums_kernel", e=e)


GN_ON = {
    # family: (record set, Cout, conv arguments, overrides, kernel)
    "mfma_64_8_8": ("cat64p_192q", 64, dict(), dict(tile=(64, 8, 8)), "conv_mfma_kernel<ConvCfg<64, 8, 8,"),
    "mfma_64_8_8_pairs": ("pairs64", 64, dict(), dict(tile=(64, 8, 8)), "conv_mfma_kernel<ConvCfg<64, 8, 8,"),
    "mfma_128_8_32": ("cat132_124", 128, dict(), dict(tile=(128, 8, 32)), "conv_mfma_kernel<ConvCfg<128, 8, 32,"),
    "mfma_adm64": ("adm64", 64, dict(), dict(tile=(64, 8, 8)), "conv_mfma_kernel<ConvCfg<64, 8, 8,"),
    "conv8": ("quads128", 128, dict(), dict(tile=(128, 16, 32)), "conv8_mfma_kernel<ConvCfg<128, 16, 32,"),      # 512 threads: 16 lanes per group
    "s2": ("pairs64", 64, dict(resample=3), dict(resident=0), "conv_s2_mfma_kernel<ConvCfg<64, 8, 8,"),
    "resident": ("pairs64", 64, dict(), dict(resident=1), "conv_resident_kernel<ResCfg<64, 8, 8,"),
    "resident_256": ("quads256", 64, dict(), dict(resident=1), "conv_resident_kernel<ResCfg<64, 8, 8,"),
    "wino": ("wino128", 128, dict(wino=True), dict(wino1=0), "conv_wino_kernel<WinoCfg<4>, false, true>"),
    "small_cout": ("pairs64_64x64", 2, dict(), dict(), "conv_small_cout_kernel"),
    "tiles180": ("tiles180", 64, dict(), dict(tile=(64, 8, 32)), "conv_mfma_kernel<ConvCfg<64, 8, 32,"),
    "c8g2": ("c8g2", 64, dict(), dict(tile=(64, 8, 32)), "conv_mfma_kernel<ConvCfg<64, 8, 32,"),
}
GN_ON_CASES = [(f, src) for f, v in GN_ON.items() for src in ("synthetic", "real") if src == "synthetic" or SETS[v[0]]["real"]]


@pytest.mark.parametrize("family,source", GN_ON_CASES)
def test_conv_with_rows_from_records(lib, family, source):
    """gn_on: a conv of every family that stages transform rows derives them itself from the records (stage_coef_rows).  Against the
    fp64 conv of silu(group_norm(x)), and against the same conv fed the table that gn_coef_from_sums_kernel wrote from the same
    records (another lane partition of the same fp64 merge: close, not bit-equal)."""
    name, Cout, cargs, ov, kernel = GN_ON[family]
    s, r = SETS[name], record_set(lib, name, source)
    Ca, C = s["parts"][0][0], r["C"]
    tag = f"gnrec/gn_on/{family}"
    rs, wino = cargs.get("resample", 0), cargs.get("wino", False)
    w, b = fx.randn(tag + "/w", Cout, C, 3, 3) / math.sqrt(C * 9), 0.1 * fx.randn(tag + "/b", Cout)
    xin = F.silu(r["ref"])
    ref = (F.conv2d(F.pad(xin, (0, 1, 0, 1)), w.double(), b.double(), stride=2) if rs == 3 else F.conv2d(xin, w.double(), b.double(), padding=1))
    xa, xb = dev(r["xs"][0]), (dev(r["xs"][1]) if len(r["xs"]) > 1 else None)
    wpk, bpk = lib.op_pack_conv(dev(w), dev(b))
    table = lib.op_pack_conv_wino(dev(w)) if wino else None
    with overrides(lib, **ov):
        out, names = profiled(lib, lambda: lib.op_conv_gn(xa, xb, r["recs"][0], r["tilings"][0], s["groups"], dev(r["gamma"]), dev(r["beta"]),
                                                         wpk, bpk, Cout, 3, act=1, wino=table, resample=rs, **gn_kwargs(s, r)))
        coef, _ = coef_table(lib, name, r)
        if wino:
            via_table = lib.op_conv_wino(xa, xb, table, bpk, Cout, coef=coef, act=1)
        else:
            via_table = lib.op_conv(xa, xb, wpk, bpk, Cout, 3, coef=coef, act=1, resample=rs)
    what = f"gn_on {family} ({source} records of {name})"
    ran(names, kernel, what)
    assert not any(n.startswith("gn_coef") for n in names), (what, names)
    e1 = close(out, ref, what + ": vs fp64")
    e2 = close(out, via_table.cpu(), what + ": vs the same conv on gn_coef_from_sums_kernel's table")
    print(f"{what}: err / bound {e1:.3e} vs fp64, {e2:.3e} vs the table path")
    note("stage_coef_rows in " + kernel.split("<")[0], e=max(e1, e2))


# ------------------------------------------------------------------------------------------------ chain
@pytest.mark.parametrize("C,H,W,rc,groups,ov,kernel", [
    (64, 16, 16, 2, 32, dict(resident=1), "conv_resident_kernel<ResCfg<64, 8, 8,"),          # GroupNorm(32): 2-channel groups
    (64, 16, 16, 2, 16, dict(resident=1), "conv_resident_kernel<ResCfg<64, 8, 8,"),          # min(32, C / 4): comparable with mcedm_op_gn_coef
    (128, 40, 24, 4, 32, dict(tile=(128, 8, 16)), "conv_mfma_kernel<ConvCfg<128, 8, 16,"),
])
def test_producer_records_consumer_chain(lib, C, H, W, rc, groups, ov, kernel):
    """conv (large-mean output y1, records) -> conv with rows from those records, against the fp64 two-conv reference, and against the
    same chain with mcedm_op_gn_coef, a pass over the tensor, in the middle (where its min(32, C / 4) groups are the ones asked).

    The bar against the two-conv reference.  y1 is an fp32 tensor of magnitude 30 and spread 1: the producer may be off by the parity
    bar there (check (b): 1e-5 + 1e-4 |y1| = 3e-3; fp32 accumulation onto a bias of 30 gives some 1e-5), and the fp64 GroupNorm itself
    turns a deviation d of y1 into d * rstd * gamma of the normalised tensor, which a unit-gain conv passes on: no consumer can be
    closer to the two-conv reference than that.  So the consumer is held to the parity bar on top of what the producer's deviation does
    to the reference itself, |f64(y1 as stored) - f64(y1 exact)| with f64 the second stage in fp64 -- computed, not estimated -- and
    the producer to the parity bar by itself.  The end-to-end figure is printed for the record."""
    tag = f"gnrec/chain/{C}_{rc}"
    t, y1 = conv_case(tag, 2, C, 0, C, H, W, 3, transform=False, sign=-1.0 if rc == 4 else 1.0)
    gamma, beta = 1 + 0.2 * fx.randn(tag + "/g", C), 0.2 * fx.randn(tag + "/be", C)
    w2, b2 = fx.randn(tag + "/w2", C, C, 3, 3) / math.sqrt(C * 9), 0.1 * fx.randn(tag + "/b2", C)

    def stage2(y):
        return F.conv2d(F.silu(F.group_norm(y, groups, gamma.double(), beta.double(), EPS)), w2.double(), b2.double(), padding=1)

    ref = stage2(y1)
    wpk2, bpk2 = lib.op_pack_conv(dev(w2), dev(b2))
    with overrides(lib, **ov):
        out1, rec, tiling, names1, _ = run_conv_case(lib, t, rc)
        out2, names2 = profiled(lib, lambda: lib.op_conv_gn(out1, None, rec, tiling, groups, dev(gamma), dev(beta), wpk2, bpk2, C, 3, act=1, eps=EPS))
        via_pass = None
        if groups == min(32, C // 4):
            coef = lib.op_gn_coef(out1, None, dev(gamma), dev(beta), eps=EPS)
            via_pass = lib.op_conv(out1, None, wpk2, bpk2, C, 3, coef=coef, act=1)
    what = f"chain {C} channels at {H} x {W}, rc={rc}, {groups} groups"
    ran(names1, kernel, what + " (producer)")
    ran(names2, kernel, what + " (consumer)")
    assert len(names2) == 1, (what, names2)
    gm, gr = R.group_stats64(y1, groups, EPS)
    assert float((gm.abs() * gr).min()) > 20, what
    close(out1, y1, what + ": producer vs fp64")
    carried = (stage2(out1.cpu().double()) - ref).abs()          # what the producer's own deviation does to the reference
    err = (out2.cpu().double() - ref).abs()
    bar = ATOL + RTOL * ref.abs()
    e = float(((err - carried).clamp_min(0) / bar).max())
    print(f"{what}: end to end max err {float(err.max()):.3e} = {float((err / bar).max()):.2f} x the parity bar, of which carried over from "
          f"the producer up to {float(carried.max()):.3e}; the consumer's own share / bar {e:.3e}")
    assert bool((err <= bar + carried).all()), f"{what}: vs the fp64 two-conv reference: consumer's share / bar {e:.3e}, max err {float(err.max()):.3e}"
    if via_pass is not None:
        e = max(e, close(out2, via_pass.cpu(), what + ": vs the chain with gn_coef_kernel in the middle"))
    note("chain through " + kernel.split("<")[0], e=e)
