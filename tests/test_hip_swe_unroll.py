"""GPU: the SWE solver unrolled on the device (mcedm_swe_fv_unroll; SweFvLoss.unroll_from_init / unroll_loss and the modules'
print_unroll_metrics) against the reference's own runs (tests/golden/swe_unroll*.npz, written by tools/make_golden_swe_unroll.py)
and against a loop of the one-step kernel.  Tensors are compared bit for bit: the kernel evaluates the same device function as
mcedm_swe_fv_step, in the same translation unit, without fma contraction.  Only the four logged scalars of print_unroll_metrics,
whose sums run in another order on the device, are held to the project's bar (rtol 1e-4, atol 1e-5)."""
import pytest
import torch

from oracle import fixtures as fx
from tests import _ddpm_edm as D
from tests import _swe_unroll as U
from tests.test_hip_module import wrap

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pde():
    import mcedm_amd  # noqa: F401
    from mcedm_amd import pde_loss
    assert torch.cuda.is_available()
    return pde_loss


def same(a, b):
    """torch.equal, except that NaNs at the same positions count as equal (infinities must agree in sign like any value)."""
    a, b = torch.as_tensor(a).cpu(), torch.as_tensor(b).cpu()
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.all((a == b) | (torch.isnan(a) & torch.isnan(b))))


def stored(golden, system, X, n):
    ic = torch.from_numpy(golden("swe_unroll.npz")[f"ic::{X}"])
    return ic, torch.from_numpy(golden(U.file_of(system, X, n))[f"unroll::{system}::{X}x{n}"])


@pytest.mark.parametrize("system", list(U.SYSTEMS))
@pytest.mark.parametrize("case", U.CASES, ids=lambda c: f"{c[0]}x{c[1]}")
def test_unroll_from_init_equals_the_reference(golden, pde, system, case):
    X, n = case
    ic, ref = stored(golden, system, X, n)
    out = pde.SweFvLoss(**U.SYSTEMS[system]).unroll_from_init(ic.cuda(), n)
    assert out.dtype == torch.float32 and tuple(out.shape) == (U.B, n + 1, X, 2)
    assert bool(torch.isfinite(ref).all()) and torch.equal(out.cpu(), ref)


@pytest.mark.parametrize("system", list(U.SYSTEMS))
def test_unstable_unroll_propagates_nan_and_inf_like_the_reference(golden, pde, system):
    X, n = U.UNSTABLE
    ic, ref = stored(golden, system, X, n)
    out = pde.SweFvLoss(**U.SYSTEMS[system]).unroll_from_init(ic.cuda(), n).cpu()
    if system == "swe":
        assert bool(torch.isnan(ref).any()) and bool(torch.isinf(ref).any())
    assert torch.equal(torch.isnan(out), torch.isnan(ref)) and same(out, ref)


@pytest.mark.parametrize("system,X,n", [("swe", 128, 127), ("swe", 127, 64), ("swe_per", 512, 127)])
def test_unroll_equals_a_loop_of_single_steps_on_the_device(pde, system, X, n):
    f = pde.SweFvLoss(**U.SYSTEMS[system])
    ic = U.initial_condition(f"loop/{system}/{X}", 8, X).cuda()
    rows, cur = [ic], ic
    for _ in range(n):
        cur = f.f_t_swp1d(cur, f.Tn / n)
        rows.append(cur)
    loop = torch.cat(rows, dim=1)
    out = f.unroll_from_init(ic, n)
    assert bool(torch.isfinite(loop).all()) and torch.equal(out, loop)
    # SweSimulatorLoss is the same class under another name (models/loss_helper.py:3-11)
    assert torch.equal(pde.SweSimulatorLoss(**U.SYSTEMS[system]).unroll_from_init(ic, n), loop)


@pytest.mark.parametrize("system", list(U.SYSTEMS))
@pytest.mark.parametrize("flip", [False, True])
def test_unroll_loss_equals_the_reference(golden, pde, system, flip):
    g = golden("swe_unroll.npz")
    pred, gt = torch.from_numpy(g[f"loss::{system}::pred"]).cuda(), torch.from_numpy(g[f"loss::{system}::gt"]).cuda()
    nh, nu = U.Norm(U.LOSS_DIVIDE[0], "cuda"), U.Norm(U.LOSS_DIVIDE[1], "cuda")
    f = pde.SweFvLoss(flip_xy=flip, **U.SYSTEMS[system])
    # with flip_xy the state arrives as (u, h), and the normalisers in that order (models/pde_loss.py:6-17, 199-209)
    args = (pred.flip(-1), gt.flip(-1), nu, nh) if flip else (pred, gt, nh, nu)
    loss, unrolled = f.unroll_loss(*args, return_unroll=True)
    only = f.unroll_loss(*args)
    assert torch.is_tensor(only) and torch.equal(only, loss)
    assert torch.equal(unrolled.cpu(), torch.from_numpy(g[f"loss::{system}::flip{int(flip)}::unrolled"]))
    assert torch.equal(loss.cpu(), torch.from_numpy(g[f"loss::{system}::flip{int(flip)}::loss"]))
    # the fused residual is what torch forms on the device from the kernel's own unroll
    scale = f.get_scaling(args[2], args[3])
    assert torch.equal(loss, (unrolled - gt) ** 2 / scale)
    # the scales are not interchangeable: the other order gives another loss
    assert not torch.equal(f.unroll_loss(args[0], args[1], args[3], args[2]), loss)


def test_initial_condition_is_read_in_place(golden, pde):
    from mcedm_amd import lib as L
    g = golden("swe_unroll.npz")
    pred = torch.from_numpy(g["loss::swe_per::pred"]).cuda()
    assert tuple(pred.shape) == (3, 9, 16, 2)
    f = pde.SweFvLoss(**U.SYSTEMS["swe_per"])
    keep = pred.clone()
    view = pred[:, 0:1]
    assert not view.is_contiguous()
    a = f.unroll_from_init(view, 8)
    b = f.unroll_from_init(view.contiguous(), 8)
    assert torch.equal(a, b) and torch.equal(pred, keep)
    # the binding passes the view's own pointer and stride: through the C entry with pred's address the result is the same
    out = torch.empty_like(a)
    half_dt, dx = float(torch.tensor(0.5 * (f.Tn / 8), dtype=torch.float32)), f._dx(16)
    L.check(L.load().mcedm_swe_fv_unroll(pred.data_ptr(), pred.stride(0), out.data_ptr(), None, None, 3, 8, 16, half_dt, dx, 1.0, 1.0,
                                         torch.cuda.current_stream().cuda_stream))
    assert torch.equal(out, a)
    # (b, x, 2) rows are accepted like (b, 1, x, 2); n_steps == 0 through the binding copies the initial condition
    assert torch.equal(L.swe_fv_unroll(pred[:, 0], 8, half_dt, dx), a)
    assert torch.equal(L.swe_fv_unroll(view, 0, half_dt, dx), view)


def test_c_call_is_captured_in_a_graph(pde):
    from mcedm_amd import lib as L
    f = pde.SweFvLoss(**U.SYSTEMS["swe_per"])
    Bn, X, n = 4, 65, 33
    half_dt, dx = float(torch.tensor(0.5 * (f.Tn / n), dtype=torch.float32)), f._dx(X)
    ic0, ic1 = (U.initial_condition(f"graph/{k}", Bn, X).cuda() for k in (0, 1))
    gt = U.initial_condition("graph/gt", Bn, X).cuda().repeat(1, n + 1, 1, 1).contiguous()
    ic = ic0.clone()
    out, loss = torch.empty(Bn, n + 1, X, 2, device="cuda"), torch.empty(Bn, n + 1, X, 2, device="cuda")
    lib = L.load()

    def call():
        L.check(lib.mcedm_swe_fv_unroll(ic.data_ptr(), 2 * X, out.data_ptr(), gt.data_ptr(), loss.data_ptr(), Bn, n, X, half_dt, dx,
                                        0.49, 1.69, torch.cuda.current_stream().cuda_stream))

    call()                                       # once outside the capture: the code object is loaded
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    ic.copy_(ic1)
    out.zero_()
    loss.zero_()
    graph.replay()
    want_loss, want = L.swe_fv_unroll(ic1, n, half_dt, dx, gt, (0.49, 1.69))
    assert torch.equal(out, want) and torch.equal(loss, want_loss)
    assert not torch.equal(want, L.swe_fv_unroll(ic0, n, half_dt, dx))


def test_print_unroll_metrics_equals_the_reference(golden):
    import mcedm_amd  # noqa: F401
    from mcedm_amd.ddim import PlCondEdm
    g = golden("swe_unroll.npz")
    m = D.fill(PlCondEdm(wrap(D.hparams_dict())).cuda(), 1, fx.STEP_NORM_STATS)
    m.set_pde_loss_function(U.METRIC_SYSTEM, False)
    logs = {}
    m.log = lambda name, value, **k: logs.__setitem__(name, torch.as_tensor(value).detach().cpu())
    xs, h_unnorm, u_unnorm, state_gt = (torch.from_numpy(g[f"metric::{k}"]).cuda() for k in ("xs", "h_unnorm", "u_unnorm", "state_gt"))
    assert tuple(xs.shape) == (U.METRIC_N * U.METRIC_B, 1, U.METRIC_T, U.METRIC_X, 1)
    before = m.pde_loss
    res, res_gt = m.print_unroll_metrics(xs, h_unnorm, u_unnorm, state_gt, U.METRIC_N)
    assert m.pde_loss is m.pde_loss_simulator and m.pde_loss is not before
    assert tuple(res.shape) == (U.METRIC_B, 1, U.METRIC_T, U.METRIC_X, U.METRIC_N, 2)
    assert torch.equal(res.cpu(), torch.from_numpy(g["metric::unroll_res"]))
    assert torch.equal(res_gt.cpu(), torch.from_numpy(g["metric::unroll_res_gt"]))
    assert sorted(logs) == sorted(U.METRIC_LOGS)
    for k in U.METRIC_LOGS:
        ref = torch.from_numpy(g[f"metric::log::{k}"])
        print(f"{k}: device {float(logs[k]):.8g}, reference {float(ref):.8g}")
        torch.testing.assert_close(logs[k], ref, rtol=1e-4, atol=1e-5, msg=lambda s: f"{k}: {s}")
    # get_x_unnorm: 'b c h w' inputs are rearranged first
    h, u = state_gt[..., 0:1], state_gt[..., 1:2]
    assert torch.equal(m.get_x_unnorm(h.permute(0, 3, 1, 2), u.permute(0, 3, 1, 2)), m.get_x_unnorm(h, u, do_rearrange=False))
