"""The SPLIT variant of the Winograd kernel (csrc/conv_wino.hip, WinoSplitCfg): the un-resampled 3x3 convs of images below 32 x 32.  A
workgroup is one 32-channel output block x one 8 x 16-pixel tile x all sixteen positions, the positions split over its eight waves;
the input path is WinoCfg<4>'s, every position sums its chunks in the same order and the epilogue evaluates the output transform in
the existing kernel's expression tree, so outputs and fused GroupNorm records must carry the bits of conv_wino_kernel<WinoCfg<4>> /
<WinoCfg<2>> on the same shape.

  1. bit identity against the existing kernel (mcedm_op_conv_wino_sums against mcedm_op_conv_wino_split_sums): four shapes x
     activation on / off x residual none / same-size / RS_DOWN, the kernels named by the profiler.  The existing kernel serves whole
     64-channel blocks only, so for Cout = 32 and 96 its arm runs on weights, bias and residual zero-padded to 64 and 128 channels and
     the first Cout channels (and their records) are compared: a channel's sum never depends on the other channels of the launch.
  2. against fp64 at the bar of tests/_tol.py (rtol 1e-4, atol 1e-5 x max|sample|), shapes 2 and 3;
  3. rows of a B = 3 launch equal the B = 1 launches bit for bit, records included;
  4. the dispatcher: a folded skip projection, an 8 x 8 image, a 32 x 32 image and a misaligned input keep their kernels with the switch
     on; an aligned 16 x 16 launch takes the new kernel, unless the input-resident switch is set explicitly;
  5. one inference forward of a ch = 32, ch_mult (1, 1, 1) plan at 64 x 64 (its last level is 16 x 16), B = 2: switch on against off
     at the bar of tests/_tol.py, switch off launches the kernels recorded before the variant existed (and an untouched plan those of
     one of the two arms), graph replay == eager with the switch on."""
import pytest
import torch

from oracle import fixtures as fx
from oracle import mcedm_oracle as orc
from tests import _tol

pytestmark = pytest.mark.gpu

RS_NONE, RS_DOWN = 0, 2
SPLIT = "conv_wino_kernel<WinoSplitCfg, false, {act}>"
# (B, Ca, Cb, Cout, H, W)
SHAPES = {
    "one_tile": (2, 16, 0, 32, 8, 16),            # one tile, one stage
    "two_tiles_cat": (2, 24, 8, 64, 16, 16),      # two tiles, two output blocks, concatenated input, four chunks
    "workload": (3, 128, 0, 128, 16, 16),         # the workload's channel counts at B = 3
    "odd_chunks": (1, 40, 0, 96, 8, 32),          # five chunks: the last stage is half full
}
RES = ("none", "same", "down")
# launches of one inference forward of the small plan of test 5 BEFORE the variant existed (recorded from the parent commit's build)
SMALL_PLAN_LAUNCHES_WITHOUT = {
    "act_materialize_kernel": 2, "conv_mfma_kernel<ConvCfg<32, 8, 32, 1, 4, 9, 8, 256, 1>, 0>": 8,
    "conv_mfma_kernel<ConvCfg<32, 8, 32, 1, 4, 9, 8, 256, 1>, 1>": 2, "conv_mfma_kernel<ConvCfg<32, 8, 8, 1, 2, 9, 8, 256, 1>, 0>": 12,
    "conv_resident_kernel<ResCfg<32, 8, 16, 1, 4, 9, 8, 1>, 0, true>": 9, "conv_small_cout_kernel": 1, "gn_coef_from_sums_kernel": 2}


@pytest.fixture(scope="module")
def lib():
    import importlib
    L = importlib.import_module("m-cedm_amd.lib")
    L.load()
    return L


def dev(t):
    return None if t is None else t.cuda().contiguous()


def inputs(name, act, res):
    B, Ca, Cb, Cout, H, W = SHAPES[name]
    tag, Cin = f"wino_split/{name}", Ca + Cb
    coef = torch.stack([fx.randn(tag + "/m", B, Cin) * 0.1, 1 + 0.1 * fx.randn(tag + "/s", B, Cin), 0.1 * fx.randn(tag + "/o", B, Cin),
                        torch.zeros(B, Cin)], -1) if act else None          # act = 0: a materialised input, as the down block's conv0 reads it
    r = None if res == "none" else fx.randn(tag + "/res/" + res, B, Cout, *((H, W) if res == "same" else (2 * H, 2 * W)))
    return dict(xa=fx.randn(tag + "/xa", B, Ca, H, W), xb=fx.randn(tag + "/xb", B, Cb, H, W) if Cb else None,
                w=fx.randn(tag + "/w", Cout, Cin, 3, 3) / (Cin * 9) ** 0.5, b=fx.randn(tag + "/b", Cout) * 0.1, coef=coef, res=r)


def reference(name, act, res, t):
    """fp64: torch's direct convolution of the activated input, plus the residual (RS_DOWN: the 2x2 mean of its source)."""
    x = (torch.cat([t["xa"], t["xb"]], 1) if t["xb"] is not None else t["xa"]).double()
    if t["coef"] is not None:
        c = t["coef"].double()
        x = (x - c[..., 0, None, None]) * c[..., 1, None, None] + c[..., 2, None, None]
    if act:
        x = torch.nn.functional.silu(x)
    ref = torch.nn.functional.conv2d(x, t["w"].double(), t["b"].double(), padding=1)
    if res == "same":
        ref = ref + t["res"].double()
    if res == "down":
        ref = ref + torch.nn.functional.avg_pool2d(t["res"].double(), 2)
    return ref


def profiled(L, fn):
    L.prof_enable(True)
    try:
        out = fn()
        torch.cuda.synchronize()
        names = sorted({r["name"] for r in L.prof_report()})
    finally:
        L.prof_enable(False)
    return out, names


def records(gsum, B, H, W, C):
    """The flat table of a Winograd launch as [B, tiles, C / 4, 2] (8 x 16-pixel tiles, 4-channel blocks)."""
    tiles = (H // 8) * (W // 16)
    return gsum[:B * tiles * (C // 4) * 2].view(B, tiles, C // 4, 2)


def run_split(L, name, act, res, t=None, rows=slice(None)):
    B, Ca, Cb, Cout, H, W = SHAPES[name]
    t = t or inputs(name, act, res)
    cut = lambda v: None if v is None else dev(v[rows])
    (out, gsum), names = profiled(L, lambda: L.op_conv_wino_split(
        cut(t["xa"]), cut(t["xb"]), L.op_pack_conv_wino(dev(t["w"])), dev(t["b"]), Cout, coef=cut(t["coef"]), act=act, res=cut(t["res"]),
        res_mode=RS_DOWN if res == "down" else RS_NONE, want_sums=True))
    return out.cpu(), records(gsum, out.shape[0], H, W, Cout).cpu(), names


def run_existing(L, name, act, res):
    """The existing kernel on the same shape; Cout padded with zero channels to its 64-channel granule where needed."""
    B, Ca, Cb, Cout, H, W = SHAPES[name]
    t = inputs(name, act, res)
    Cp = (Cout + 63) // 64 * 64
    pad = lambda v, dim: None if v is None else torch.cat([v, torch.zeros(*v.shape[:dim], Cp - Cout, *v.shape[dim + 1:])], dim) if Cp != Cout else v
    (out, gsum), names = profiled(L, lambda: L.op_conv_wino(
        dev(t["xa"]), dev(t["xb"]), L.op_pack_conv_wino(dev(pad(t["w"], 0))), dev(pad(t["b"], 0)), Cp, coef=dev(t["coef"]), act=act,
        res=dev(pad(t["res"], 1)), res_mode=RS_DOWN if res == "down" else RS_NONE, want_sums=True))
    return out.cpu()[:, :Cout], records(gsum, B, H, W, Cp).cpu()[:, :, :Cout // 4], names, Cp


@pytest.mark.parametrize("res", RES)
@pytest.mark.parametrize("act", (1, 0))
@pytest.mark.parametrize("name", list(SHAPES))
def test_split_is_bit_equal_to_the_existing_winograd_kernel(lib, name, act, res):
    a, ra, na = run_split(lib, name, act, res)
    b, rb, nb, Cp = run_existing(lib, name, act, res)
    tf = "true" if act else "false"
    assert na == [SPLIT.format(act=tf)], na
    assert nb == [f"conv_wino_kernel<WinoCfg<{4 if Cp % 128 == 0 else 2}>, false, {tf}>"], nb
    print(f"{name} act {act} res {res}: {int((a != b).sum())} of {a.numel()} outputs differ, max |d| {float((a - b).abs().max()):.3e}; "
          f"{int((ra != rb).sum())} of {ra.numel()} record values differ")
    assert rb.abs().max() > 0 and torch.isfinite(a).all()
    assert torch.equal(a, b)
    assert torch.equal(torch.signbit(a), torch.signbit(b))      # -0 == +0 under equal: the zeros' signs too
    assert torch.equal(ra, rb)


@pytest.mark.parametrize("res", RES)
@pytest.mark.parametrize("act", (1, 0))
@pytest.mark.parametrize("name", ["two_tiles_cat", "workload"])
def test_split_vs_fp64(lib, name, act, res):
    t = inputs(name, act, res)
    out, _, _ = run_split(lib, name, act, res, t)
    worst = _tol.close_per_entry(out, reference(name, act, res, t), what=f"{name} act {act} res {res}: split Winograd conv vs fp64", time_dim=0)
    print(f"{name} act {act} res {res}: worst err / bar {worst:.3f}")


def test_rows_of_a_batch_equal_the_single_sample_launches(lib):
    name, act, res = "workload", 1, "same"
    t = inputs(name, act, res)
    out, rec, _ = run_split(lib, name, act, res, t)
    for b in range(SHAPES[name][0]):
        o1, r1, _ = run_split(lib, name, act, res, t, rows=slice(b, b + 1))
        assert torch.equal(o1[0], out[b]), (b, float((o1[0] - out[b]).abs().max()))
        assert torch.equal(r1[0], rec[b]), b


def dispatched(L, flag, fn, resident=-1):
    """fn() through the dispatcher with the split switch at `flag` -> (outputs, kernel names)."""
    L.set_conv_wino_split(flag)
    L.set_conv_resident(resident)
    try:
        return profiled(L, fn)
    finally:
        L.set_conv_wino_split(-1)
        L.set_conv_resident(-1)


def conv_launch(L, tag, B, Cin, Cout, H, W, misalign=False):
    """A 3x3 conv with a Winograd table through the dispatcher (mcedm_op_conv_sums), as a plan launches it."""
    w, b = dev(fx.randn(tag + "/w", Cout, Cin, 3, 3) / (Cin * 9) ** 0.5), dev(fx.randn(tag + "/b", Cout) * 0.1)
    wpk, bpk = L.op_pack_conv(w, b)
    wino = L.op_pack_conv_wino(w)
    x = dev(fx.randn(tag + "/x", B, Cin, H, W))
    if misalign:          # the same values 4 bytes off a 16-byte boundary
        buf = torch.empty(x.numel() + 1, dtype=torch.float32, device="cuda")
        buf[1:] = x.flatten()
        x = buf[1:].view(x.shape)
        assert x.data_ptr() % 16 == 4
    return lambda: L.op_conv_sums(x, None, wpk, bpk, Cout, 3, wino=wino)[0]


def skip_launch(L, tag, B, Cin, Csk, Cout, H, W):
    """conv1 of a decoder block with its 1x1 skip projection folded in (mcedm_op_conv_skip with sk_wpk)."""
    w, b = dev(fx.randn(tag + "/w", Cout, Cin, 3, 3) / (Cin * 9) ** 0.5), dev(fx.randn(tag + "/b", Cout) * 0.1)
    ws, bs = dev(fx.randn(tag + "/ws", Cout, Csk, 1, 1) / Csk ** 0.5), dev(fx.randn(tag + "/bs", Cout) * 0.1)
    wpk, bpk = L.op_pack_conv(w, b)
    swpk, sbpk = L.op_pack_conv(ws, bs)
    wino = L.op_pack_conv_wino(w)
    x, sk = dev(fx.randn(tag + "/x", B, Cin, H, W)), dev(fx.randn(tag + "/sk", B, Csk, H, W))
    return lambda: L.op_conv_skip(x, wpk, wino, bpk, Cout, sk_xa=sk, sk_wpk=swpk, sk_bias=sbpk)


@pytest.mark.parametrize("case", ["folded_skip", "8x8", "32x32", "misaligned"])
def test_dispatcher_keeps_the_kernels_of_launches_the_variant_does_not_serve(lib, case):
    tag = "wino_split/disp/" + case
    fn = {"folded_skip": lambda: skip_launch(lib, tag, 2, 64, 32, 64, 16, 16),
          "8x8": lambda: conv_launch(lib, tag, 2, 64, 64, 8, 8),
          "32x32": lambda: conv_launch(lib, tag, 2, 64, 64, 32, 32),
          "misaligned": lambda: conv_launch(lib, tag, 2, 64, 64, 16, 16, misalign=True)}[case]()
    on, n_on = dispatched(lib, 1, fn)
    off, n_off = dispatched(lib, 0, fn)
    print(case, n_on)
    assert n_on == n_off and not any("WinoSplitCfg" in n for n in n_on), (n_on, n_off)
    if case == "32x32":
        assert n_on == ["conv_wino_kernel<WinoCfg<2>, false, false>"], n_on
    assert torch.equal(on, off)


def test_dispatcher_gives_an_aligned_16x16_launch_to_the_variant(lib):
    fn = conv_launch(lib, "wino_split/disp/16x16", 2, 64, 64, 16, 16)
    on, n_on = dispatched(lib, 1, fn)
    off, n_off = dispatched(lib, 0, fn)
    res, n_res = dispatched(lib, 1, fn, resident=1)              # an explicit request for the input-resident kernels wins
    assert n_on == [SPLIT.format(act="false")], n_on
    assert len(n_off) == 1 and n_off[0].startswith("conv_resident_kernel<ResCfg<64, 8, 8,"), n_off
    assert n_res == n_off and torch.equal(res, off), n_res
    worst = _tol.close_per_entry(on, off, what="16 x 16 conv: split Winograd against the input-resident kernel", time_dim=0)
    print(f"split vs resident: worst err / bar {worst:.3f}")


def test_inference_forward_of_a_small_plan(lib):
    cfg = orc.UNetConfig(ch=32, ch_mult=(1, 1, 1), attn_resolutions=(16,), resolution=64)
    mk = lambda: lib.Plan(cfg.in_channels, cfg.cond_channels, cfg.out_ch, cfg.ch, cfg.ch_mult, cfg.num_res_blocks,
                          cfg.attn_resolutions, cfg.resolution)
    P = {k: v.cuda() for k, v in orc.make_params(cfg, 7).items()}
    x = fx.randn("wino_split/plan/x", 2, cfg.in_channels, 64, 64).cuda()
    cond = fx.randn("wino_split/plan/c", 2, cfg.cond_channels, 64, 64).cuda() if cfg.cond_channels else None
    sig = torch.tensor([0.5, 2.0]).cuda()
    got = {}
    for flag in (1, 0, -1):          # -1: a plan nobody touched
        plan = mk()
        if flag >= 0:
            plan.set_variant("conv_wino_split", flag)
        packed = plan.pack(P)
        lib.prof_enable(True)
        try:
            D = plan.denoise(packed, x, sig, cond=cond)
            torch.cuda.synchronize()
            rows = {r["name"]: int(r["launches"]) for r in lib.prof_report()}
        finally:
            lib.prof_enable(False)
        got[flag] = (D.cpu(), rows, plan, packed)
    k_split = SPLIT.format(act="true")
    print("switch on:", {k: v for k, v in got[1][1].items() if "Wino" in k})
    assert got[1][1].get(k_split, 0) >= 1, got[1][1]
    assert got[0][1] == SMALL_PLAN_LAUNCHES_WITHOUT, got[0][1]
    default_on = any("WinoSplitCfg" in k for k in got[-1][1])
    # the switch's two positions are the two sets of launches there are: an untouched plan runs one of them
    assert got[-1][1] == got[1 if default_on else 0][1], (got[-1][1], got[0][1])
    assert torch.equal(got[-1][0], got[1 if default_on else 0][0])
    worst = _tol.close_per_entry(got[1][0], got[0][0], what="small plan: switch on against off", time_dim=0)
    print(f"small plan, switch on / off: worst err / bar {worst:.3f}, max |d| {float((got[1][0] - got[0][0]).abs().max()):.3e}")
    # graph replay == eager with the switch on: same workspace, same static inputs
    _, _, plan, packed = got[1]
    ws = lib.Workspace()
    eager = plan.denoise(packed, x, sig, cond=cond, ws=ws).clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        Dg = plan.denoise(packed, x, sig, cond=cond, ws=ws)
    Dg.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(Dg, eager), float((Dg - eager).abs().max())
    assert torch.equal(eager.cpu(), got[1][0])
