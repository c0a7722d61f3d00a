"""CPU: the PDE term of training (optimization.pde_loss_lambda > 0, models/ddim.py:1726-1731).  The torch restatement of
tests/_pde_train.py reproduces the reference's get_pde_loss values and gradients (tests/golden/pde_train.npz), the header declares
the entry and the binding carries it, and the drop-ins take the three knobs."""
import numpy as np
import pytest
import torch

import mcedm_amd  # noqa: F401
from oracle import fixtures as fx
from tests import _pde_train as T
from tests.test_cond_ddim_cpu import ddim_hparams
from tests.test_hip_cond_edm import cond_hparams
from tests.test_hip_module import hparams


@pytest.mark.parametrize("name", list(T.OP_CASES))
def test_restatement_reproduces_the_reference(golden, name):
    """fp32, the reference's own arithmetic: the value to summation order, the gradient to a few ulp of its largest entry; entries
    the reference returns as exactly 0 (clamped cells, the cancelled row 0) and as NaN (the dry cell) are the same entries."""
    g = golden("pde_train.npz")
    c = T.OP_CASES[name]
    val, grad = T.restate(c["system"], *T.op_inputs(name), stats=c["stats"])
    ref_v, ref_g = torch.as_tensor(g[f"{name}::value"]), torch.as_tensor(g[f"{name}::grad"])
    torch.testing.assert_close(val, ref_v, rtol=1e-5, atol=0, equal_nan=True)
    torch.testing.assert_close(grad, ref_g, rtol=1e-5, atol=1e-6 * float(ref_g.nan_to_num().abs().max()), equal_nan=True)
    assert torch.equal(grad == 0, ref_g == 0)


def test_the_case_table_is_the_one_the_fixture_holds(golden):
    g = golden("pde_train.npz")
    assert {k.split("::")[0] for k in g if k.endswith("::value")} == set(T.OP_CASES)
    assert int(g["reference_training_step_raises"]) == 1       # models/ddim.py:1729 -> :1396, 1400: see the fixture's tool
    for name, c in T.OP_CASES.items():
        if c["degenerate"]:
            assert float(g[f"{name}::value"]) == 0.0 and not g[f"{name}::grad"].any()


def test_clamp_gradient_convention_of_the_installed_torch():
    """What the kernel's mask `L <= 1` restates: torch.clamp(max=1) passes the gradient at L == 1 and blocks it above and at NaN."""
    x = torch.tensor([0.5, 1.0, 2.0, float("nan")], requires_grad=True)
    torch.clamp(x, max=1.0).sum().backward()
    assert x.grad.tolist() == [1.0, 1.0, 0.0, 0.0]


def test_prop_t_broadcast_is_a_common_factor():
    """models/ddim.py:1415-1416: (b, t, x) / (b, 1, 1, 1) is (b, b, t, x); its sum is sum(M) * sum_i 1 / (sigma_i + 1)."""
    M, sigma = torch.rand(3, 4, 5, dtype=torch.float64), torch.rand(3, 1, 1, 1, dtype=torch.float64)
    out = M / (sigma + 1.0)
    assert tuple(out.shape) == (3, 3, 4, 5)
    torch.testing.assert_close(out.sum(), M.sum() * T.sample_weights(sigma.float()).double()[0], rtol=1e-6, atol=0)


def test_header_declares_the_entries_and_the_binding_carries_them():
    from mcedm_amd import abi, lib
    for name in ("mcedm_pde_train_loss", "mcedm_pde_train_scratch_bytes"):
        assert name in abi.PROTOS and name in lib.EXPORTS
    ret, args = abi.DECLS["mcedm_pde_train_loss"]
    assert ret == "int" and args[0] == "const mcedm_guidance_desc*" and len(args) == 18
    assert abi.DECLS["mcedm_pde_train_scratch_bytes"][0] == "size_t"
    assert callable(lib.pde_train_loss)


def test_cond_edm_constructs_and_stores_the_three_knobs():
    from mcedm_amd.ddim import PlCondEdm
    hp = cond_hparams()
    hp.optimization.update(pde_loss_lambda=0.1, pde_loss_prop_t=True, use_gt_pde=True)
    m = PlCondEdm(hp)
    assert (m.pde_loss_lambda, m.pde_loss_prop_t, m.use_gt_pde) == (0.1, True, True)
    m = PlCondEdm(cond_hparams())
    assert (m.pde_loss_lambda, m.pde_loss_prop_t, m.use_gt_pde) == (0.0, False, False)


def test_joint_model_accepts_and_ignores_the_knob():
    from mcedm_amd.mcedm import PlMcedm
    hp = hparams(fx.CFG_P)
    hp.optimization.update(pde_loss_lambda=0.1, pde_loss_prop_t=True, use_gt_pde=True)
    m = PlMcedm(hp)
    assert (m.pde_loss_lambda, m.pde_loss_prop_t, m.use_gt_pde) == (0.1, True, True)


def test_cond_ddim_still_raises():
    from mcedm_amd.ddim import PlCondDdim
    hp = ddim_hparams()
    hp.optimization.pde_loss_lambda = 0.1
    with pytest.raises(NotImplementedError, match="pde_loss_lambda"):
        PlCondDdim(hp)
