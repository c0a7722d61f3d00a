"""The Winograd kernels' steady state -- SEVERAL pixel tiles per workgroup -- and their use as a data gradient.

conv_wino_kernel / conv_wino1_kernel run as persistent workgroups that take `per` tiles of one sample as one stream of stages:
the loader runs ahead across the tile boundary, border geometry is switched per tile, only the accumulators are written out in
between.  The host picks per > 1 only above one round of the chip (> 32 768 pixels per call), so the op-level fp64 tests of
tests/test_hip_wino.py never leave per = 1.  Here MCEDM_WINO_PER (read once per process) forces 2 and 4 in child processes on
small shapes; every workgroup's debug record proves which schedule ran; the outputs are held to fp64 (rtol 1e-4 / atol 1e-5)
AND to the bits of the per = 1 run of this process ("results never depend on it", csrc/conv_wino.hip wino_tiles_per_wg).

Second half: the transposed, tap-mirrored table of launch_pack_conv_wino(.., transpose_flip = 1) that the backward feeds into
the same kernel for every 3x3 data gradient, against fp64 autograd (rtol 1e-4, atol 1e-5 x max|ref|: the bar of
tests/test_hip_backward.py) and against the direct kernel's data gradient."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import _wino_per as WP

gpu = pytest.mark.gpu
FORCED = (2, 4)


def test_exact_inputs_stay_exact_in_fp32_winograd_arithmetic():
    """The premise of the exact seam test, without a GPU: with x in {-3 .. 3} and w in {-2 .. 2} every value of F(2x2, 3x3) is a
    multiple of 1/4 far below 2^24 -- U = G g G^T (|U| <= 4.5), V = B^T d B (|V| <= 12), the 24-channel sums of their products
    (<= 1296) and A^T M A -- so fp32 arithmetic in ANY order gives the integers of the direct convolution.  Emulated in fp32
    numpy with the three transforms spelled out, compared with fp64.  Ranges settled on: the ones the issue proposed."""
    t = WP.seam_inputs()
    x, w = t["x"].numpy(), t["w"].numpy()
    assert x.dtype == np.float32 and set(np.unique(x)) == set(range(-3, 4)) and set(np.unique(w)) == set(range(-2, 3))
    f32 = np.float32
    G = np.array([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], f32)
    Bt = np.array([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], f32)
    At = np.array([[1, 1, 1, 0], [0, 1, -1, -1]], f32)
    U = np.einsum("ia,ocab,jb->ocij", G, w, G).astype(f32)
    assert U.dtype == f32 and np.array_equal(U * 4, np.round(U * 4)) and np.abs(U).max() <= 4.5
    B_, Cin, H, W = x.shape
    xp = np.zeros((B_, Cin, H + 2, W + 2), f32)
    xp[:, :, 1:-1, 1:-1] = x
    # the 4 x 4 input patch of every 2 x 2 output patch: d[n, c, ty, tx, 4, 4]
    d = np.stack([np.stack([xp[:, :, i:i + H:2, j:j + W:2] for j in range(4)], -1) for i in range(4)], -2)
    V = np.einsum("ia,nctuab,jb->nctuij", Bt, d, Bt).astype(f32)
    assert V.dtype == f32 and np.abs(V).max() <= 12
    M = np.zeros((B_, U.shape[0]) + V.shape[2:], f32)
    for c in range(Cin):                                   # an fp32 running sum, one channel at a time
        M += U[None, :, c, None, None] * V[:, None, c]
        assert M.dtype == f32
    assert np.abs(M).max() <= 24 * 4.5 * 12 and np.array_equal(M * 4, np.round(M * 4))
    Y = np.einsum("ia,nctuab,jb->nctiuj", At, M, At).astype(f32).reshape(B_, U.shape[0], H, W)
    assert np.array_equal(Y.astype(np.float64), WP.seam_reference(t).numpy())


@pytest.fixture(scope="module")
def lib():
    import importlib
    L = importlib.import_module("m-cedm_amd.lib")
    L.load()
    return L


def run_child(per, path):
    """tests/_wino_per.py as a fresh process with MCEDM_WINO_PER = per -> its .npz."""
    env = dict(os.environ, MCEDM_WINO_PER=str(per))
    r = subprocess.run([sys.executable, WP.__file__, path], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return dict(np.load(path))


@pytest.fixture(scope="module")
def runs(lib, tmp_path_factory):
    """{1: this process (the default schedule: one tile per workgroup at these sizes), 2 and 4: the forced children}."""
    d = tmp_path_factory.mktemp("wino_per")
    out = {1: WP.run_all(lib)}
    for per in FORCED:
        out[per] = run_child(per, str(d / f"per{per}.npz"))
    return out


@pytest.fixture(scope="module")
def refs():
    """fp64, computed once."""
    r = {name: WP.case_reference(name, WP.case_inputs(name)) for name in WP.CASES}
    r.update({name: WP.dgrad_reference(name, WP.dgrad_inputs(name)) for name in WP.DGRAD_CASES})
    r["seam"] = WP.seam_reference(WP.seam_inputs())
    return r


def close(got, ref, what, rtol=1e-4, atol=1e-5, rel_atol=0.0):
    """tests/test_hip_wino.py's bar; rel_atol: atol as a fraction of max|ref| instead (tests/test_hip_backward.py's)."""
    got, ref = torch.as_tensor(got).detach().cpu().double(), torch.as_tensor(ref).detach().cpu().double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = (got - ref).abs()
    if rel_atol:
        atol = rel_atol * float(ref.abs().max())
    bad = err > atol + rtol * ref.abs()
    print(f"{what}: max err {float(err.max()):.3e}, max ref {float(ref.abs().max()):.3e}, worst err / bound {float((err / (atol + rtol * ref.abs())).max()):.3f}")
    assert not bad.any(), f"{what}: {int(bad.sum())}/{bad.numel()} out of tolerance, max err {err.max():.3e} (max ref {ref.abs().max():.3e})"


def assert_recorded_per(words, key, per):
    """Every workgroup of the launch recorded `per` tiles, and the launch had total / per workgroups: the records behind them
    (the buffer is sized for one tile per workgroup) were never written."""
    total = WP.total_tiles_of(key)
    assert total % per == 0 and words.shape == (total,), (key, total, per, words.shape)
    print(f"{key}: recorded tiles per workgroup {sorted(set(words[:total // per].tolist()))} in {total // per} workgroups (forced {per})")
    assert (words[:total // per] == per).all() and (words[total // per:] == 0).all(), (key, per, words.tolist())


def check_forced_run(parent, child, refs, per, key):
    """The three assertions on one call of one forced child."""
    name = key.split("@")[0]
    assert_recorded_per(child[key + "/per"], key, per)
    if name in WP.DGRAD_CASES:
        close(child[key + "/out"], refs[name], f"{key} per {per} vs fp64 autograd", rel_atol=1e-5)
    elif name == "seam":
        assert np.array_equal(child[key + "/out"].astype(np.float64), refs[name].numpy()), f"{key} per {per}: not the exact integers"
    else:
        close(child[key + "/out"], refs[name], f"{key} per {per} vs fp64")
    assert np.array_equal(child[key + "/out"], parent[key + "/out"]), f"{key}: per {per} differs from per 1 in " \
        f"{int((child[key + '/out'] != parent[key + '/out']).sum())} of {parent[key + '/out'].size} values"


@gpu
@pytest.mark.parametrize("name", list(WP.CASES) + list(WP.DGRAD_FORCED) + ["seam"])
def test_default_schedule_of_these_shapes_is_one_tile_per_workgroup(runs, refs, name):
    """The base line the children are compared with bit for bit: per = 1 (from the records), and itself within the bar of fp64."""
    assert_recorded_per(runs[1][name + "/per"], name, 1)
    if name in WP.DGRAD_CASES:
        close(runs[1][name + "/out"], refs[name], f"{name} per 1 vs fp64 autograd", rel_atol=1e-5)
    elif name == "seam":
        assert np.array_equal(runs[1][name + "/out"].astype(np.float64), refs[name].numpy())
    else:
        close(runs[1][name + "/out"], refs[name], f"{name} per 1 vs fp64")


@gpu
@pytest.mark.parametrize("per", FORCED)
@pytest.mark.parametrize("name", list(WP.CASES))
def test_forced_tiles_per_workgroup_vs_fp64_and_bit_equal_to_one_tile(runs, refs, name, per):
    check_forced_run(runs[1], runs[per], refs, per, name)


@gpu
@pytest.mark.parametrize("per", (1,) + FORCED)
@pytest.mark.parametrize("name", WP.WINO1_CASES)
def test_one_wave_per_simd_kernel_is_bit_identical_with_several_tiles_per_workgroup(runs, name, per):
    """tests/test_hip_wino.py's claim for conv_wino1_kernel, which reads the same MCEDM_WINO_PER: equal to WinoCfg<4> of the SAME
    process bit for bit -- plain, up-sampled, RS_UP and RS_DOWN residual."""
    r = runs[per]
    assert_recorded_per(r[name + "@wino1/per"], name + "@wino1", per)
    assert_recorded_per(r[name + "/per"], name, per)
    assert np.isfinite(r[name + "@wino1/out"]).all()
    assert np.array_equal(r[name + "@wino1/out"], r[name + "/out"])


@gpu
@pytest.mark.parametrize("per", FORCED)
def test_exact_integers_across_tile_seams(runs, refs, per):
    """x in {-3 .. 3}, w in {-2 .. 2}, (2, 24 -> 128, 32 x 16), no transform, no activation, no bias: every product and partial
    sum is exact in fp32 (the CPU test above), so the output must EQUAL the fp64 convolution.  Anything carried across a tile
    boundary -- a stale geometry register, the wrong tile's halo, the previous tile's border mask -- changes an integer."""
    check_forced_run(runs[1], runs[per], refs, per, "seam")


@gpu
@pytest.mark.parametrize("per", FORCED)
@pytest.mark.parametrize("name", WP.DGRAD_FORCED)
def test_winograd_data_gradient_under_a_forced_schedule(runs, refs, name, per):
    check_forced_run(runs[1], runs[per], refs, per, name)


@gpu
@pytest.mark.parametrize("name", list(WP.DGRAD_CASES))
def test_winograd_data_gradient_vs_autograd_and_direct_kernel(lib, refs, name):
    """du = conv_wino_kernel(dy, table of op_pack_conv_wino(w, dgrad=True)) against gu = autograd.grad(conv2d(u, w, padding=1),
    u, dy) in fp64 and against the direct kernel's data gradient (tests/test_hip_backward.py test_conv_wgrad_and_dgrad).  Random
    weights: a missing tap flip or channel transpose cannot cancel."""
    B, Cin, Cout, H, W = WP.DGRAD_CASES[name]
    t = WP.dgrad_inputs(name)
    w, dy = WP.dev(t["w"]), WP.dev(t["dy"])
    table = lib.op_pack_conv_wino(w, dgrad=True)
    lib.prof_enable(True)
    try:
        du = lib.op_conv_wino(dy, None, table, None, Cin)
        torch.cuda.synchronize()
        names = {r["name"] for r in lib.prof_report()}
    finally:
        lib.prof_enable(False)
    # the training step's instantiation: no activation on a raw gradient
    assert any(n.startswith("conv_wino_kernel<") and n.endswith(", false, false>") for n in names), names
    assert not any(n.startswith("conv_mfma") or n.startswith("conv_resident") for n in names), names
    close(du, refs[name], f"{name}: Winograd data gradient vs fp64 autograd", rel_atol=1e-5)
    wpk, _ = lib.op_pack_conv(w, None, dgrad=True)
    close(du, lib.op_conv(dy, None, wpk, None, Cin, 3), f"{name}: Winograd vs direct data gradient", rel_atol=1e-5)
    if Cin == Cout:       # same table size: what a forgotten transpose_flip would hand to the kernel
        fwd = lib.op_pack_conv_wino(w)
        assert fwd.shape == table.shape and not torch.equal(fwd, table)
        wrong = lib.op_conv_wino(dy, None, fwd, None, Cin)
        assert float((wrong.cpu().double() - refs[name]).abs().max()) > 0.1 * float(refs[name].abs().max())
