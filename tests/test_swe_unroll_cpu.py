"""CPU-only checks of the device-side SWE unroll (mcedm_swe_fv_unroll, SweFvLoss.unroll_from_init / unroll_loss,
print_unroll_metrics): the C entry is declared, exported and bound, it validates its arguments before any launch, the drop-in
classes carry the reference's methods and raise what the reference raises, and tests/golden/swe_unroll*.npz is the reference's:
a loop of the oracle's step over the stored inputs reproduces every stored unrolled tensor bit for bit."""
import ctypes as C
import os
import re

import pytest
import torch

import mcedm_amd  # noqa: F401
from mcedm_amd import lib as L
from mcedm_amd import ddim, pde_loss
from tests import _swe_unroll as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mcedm_hip.h")


def same(a, b):
    """torch.equal, except that NaNs at the same positions count as equal."""
    a, b = torch.as_tensor(a), torch.as_tensor(b)
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.all((a == b) | (torch.isnan(a) & torch.isnan(b))))


def test_symbol_is_declared_exported_and_bound():
    hdr = open(HEADER).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"\bint\s+mcedm_swe_fv_unroll\s*\(\s*const float\*\s*ic,\s*size_t\s+ic_sample_stride,", code)
    assert "mcedm_swe_fv_unroll" in L.EXPORTS
    fn = L.load().mcedm_swe_fv_unroll
    assert fn.restype is C.c_int and len(fn.argtypes) == 13 and fn.argtypes[1] is C.c_size_t
    consts = {k: int(v) for k, v in re.findall(r"#define (MCEDM_[A-Z0-9_]+) (\d+)\b", hdr)}
    assert consts["MCEDM_SWE_UNROLL_MAX_X"] == L.SWE_UNROLL_MAX_X == 4096
    assert 2 * L.SWE_UNROLL_MAX_X * 8 == 64 * 1024          # two rows of float2 pairs are exactly 64 KB of LDS
    assert "models/pde_loss.py:167-182" in hdr              # the entry's comment cites the reference like its neighbours


P = C.c_void_p(16)          # never dereferenced: every check below fails before a launch
MAX_X = L.SWE_UNROLL_MAX_X
#        ic,   stride, out,  gt,   loss, B, n_steps, X
BAD = [
    ((None, 64, P, None, None, 1, 3, 32), b"ic is null"),
    ((P, 64, None, None, None, 1, 3, 32), b"out is null"),
    ((P, 64, P, P, None, 1, 3, 32), b"loss is null"),
    ((P, 64, P, None, P, 1, 3, 32), b"gt is null"),
    ((P, 64, P, None, None, 1, 3, 0), b"X = 0"),
    ((P, 64, P, None, None, 1, 3, -5), b"X = -5"),
    ((P, 2 * (MAX_X + 1), P, None, None, 1, 3, MAX_X + 1), b"X = 4097"),
    ((P, 64, P, None, None, 1, -1, 32), b"n_steps = -1"),
    ((P, 64, P, None, None, -1, 3, 32), b"B = -1"),
    ((P, 63, P, None, None, 1, 3, 32), b"ic_sample_stride = 63"),
    ((P, 0, P, P, P, 2, 3, 32), b"ic_sample_stride = 0"),
]


@pytest.mark.parametrize("args,text", BAD, ids=[t.decode() for _, t in BAD])
def test_bad_arguments_are_rejected_before_any_launch(args, text):
    lib = L.load()
    ic, stride, out, gt, loss, B, n, X = args
    rc = lib.mcedm_swe_fv_unroll(ic, stride, out, gt, loss, B, n, X, 0.001, 0.03, 1.0, 1.0, None)
    msg = lib.mcedm_last_error()
    assert rc == -1 and msg.startswith(b"swe_fv_unroll: ") and text in msg, msg


def test_empty_batch_is_ok_without_a_launch():
    lib = L.load()
    assert lib.mcedm_swe_fv_unroll(P, 64, P, None, None, 0, 3, 32, 0.001, 0.03, 1.0, 1.0, None) == 0
    assert lib.mcedm_swe_fv_unroll(P, 2 * MAX_X, P, P, P, 0, 0, MAX_X, 0.001, 0.03, 1.0, 1.0, None) == 0
    # an empty batch does not excuse a bad argument
    assert lib.mcedm_swe_fv_unroll(P, 2 * MAX_X + 2, P, None, None, 0, 3, MAX_X + 1, 0.001, 0.03, 1.0, 1.0, None) == -1


def test_drop_in_classes_have_the_reference_methods():
    import inspect
    for cls in (pde_loss.SweFvLoss, pde_loss.SweSimulatorLoss):
        assert list(inspect.signature(cls.unroll_from_init).parameters) == ["self", "ic", "n_steps"]
        sig = inspect.signature(cls.unroll_loss)
        assert list(sig.parameters) == ["self", "pred", "gt", "normalizer_h", "normalizer_u", "return_unroll"]
        assert sig.parameters["return_unroll"].default is False
    assert not hasattr(pde_loss.DarcyLoss, "unroll_loss") and not hasattr(pde_loss.DarcyLoss, "unroll_from_init")
    for cls in (ddim.PlCondDdim, ddim.PlCondEdm):
        assert list(inspect.signature(cls.print_unroll_metrics).parameters) == ["self", "xs", "h_unnorm", "u_unnorm", "state_gt",
                                                                                "n_samples"]
        sig = inspect.signature(cls.get_x_unnorm)
        assert list(sig.parameters) == ["self", "cond", "x_denoised", "do_rearrange"] and sig.parameters["do_rearrange"].default is True
    for system in U.SYSTEMS:
        fv, sim = pde_loss.get_pde_loss_function(system, False)
        assert hasattr(fv, "unroll_loss") and hasattr(sim, "unroll_loss")


def test_cpu_tensors_raise_and_one_row_divides_by_zero():
    f = pde_loss.SweFvLoss(**U.SYSTEMS["swe_per"])
    nh, nu = U.Norm(0.7), U.Norm(1.3)
    pred = U.initial_condition("cpu", 2, 16).repeat(1, 9, 1, 1)
    with pytest.raises(RuntimeError, match="CPU tensor"):
        L.swe_fv_unroll(pred[:, 0:1], 8, 0.001, 0.03)
    with pytest.raises(RuntimeError, match="CPU tensor"):
        f.unroll_from_init(pred[:, 0:1], 8)
    with pytest.raises(RuntimeError, match="CPU tensor"):
        f.unroll_loss(pred, pred, nh, nu)
    # pred.shape[1] - 1 == 0 steps: the reference divides Tn by it (models/pde_loss.py:176)
    with pytest.raises(ZeroDivisionError):
        f.unroll_loss(pred[:, :1], pred[:, :1], nh, nu)
    with pytest.raises(ZeroDivisionError):
        pde_loss.SweSimulatorLoss(flip_xy=True).unroll_loss(pred[:, :1], pred[:, :1], nh, nu, return_unroll=True)


@pytest.mark.parametrize("system", list(U.SYSTEMS))
@pytest.mark.parametrize("case", U.CASES + [U.UNSTABLE], ids=lambda c: f"{c[0]}x{c[1]}")
def test_fixture_is_the_references_unroll(golden, system, case):
    X, n = case
    ic = torch.from_numpy(golden("swe_unroll.npz")[f"ic::{X}"])
    ref = torch.from_numpy(golden(U.file_of(system, X, n))[f"unroll::{system}::{X}x{n}"])
    assert tuple(ic.shape) == (U.B, 1, X, 2) and tuple(ref.shape) == (U.B, n + 1, X, 2)
    mine = U.oracle_unroll(ic, n, **U.SYSTEMS[system])
    if case == U.UNSTABLE:
        assert same(mine, ref)
        if system == "swe":
            assert bool(torch.isnan(ref).any()) and bool(torch.isinf(ref).any())
    else:
        assert bool(torch.isfinite(ref).all()) and torch.equal(mine, ref)


@pytest.mark.parametrize("system", list(U.SYSTEMS))
def test_fixture_unroll_loss_is_the_residual_of_the_unroll(golden, system):
    """The stored unroll_loss tensors: the unroll of pred[:, 0:1] by the oracle, and (unrolled - gt)^2 / (divide_h, divide_u)^2 --
    the same for flip_xy False and True, which see the physical state in the end."""
    g = golden("swe_unroll.npz")
    pred, gt = torch.from_numpy(g[f"loss::{system}::pred"]), torch.from_numpy(g[f"loss::{system}::gt"])
    assert tuple(pred.shape) == U.LOSS_SHAPE + (2,)
    unrolled = U.oracle_unroll(pred[:, 0:1], pred.shape[1] - 1, **U.SYSTEMS[system])
    scale = torch.tensor(U.LOSS_DIVIDE) ** 2
    for flip in (0, 1):
        assert torch.equal(torch.from_numpy(g[f"loss::{system}::flip{flip}::unrolled"]), unrolled)
        assert torch.equal(torch.from_numpy(g[f"loss::{system}::flip{flip}::loss"]), (unrolled - gt) ** 2 / scale)
