"""CPU-only checks of the per-sample-timestep entries of the DDPM U-Net (mcedm_ddpm_temb_rows, mcedm_ddpm_forward_t,
mcedm_ddpm_edm_denoise_t, mcedm_ddpm_workspace_bytes_t, the bias_batch forms of the two op-level conv entries): the symbols are
in the header, the binding and the library; every entry rejects bad arguments on the host, before any launch; the existing size
queries return what they returned before these entries existed; and the goldens of tests/golden/ddpm_pert.npz are what the
fp32 oracle computes."""
import ctypes as C
import os
import re
import subprocess

import pytest
import torch

import mcedm_amd  # noqa: F401
from mcedm_amd import lib as L
from tests import _ddpm_arch as A
from tests import _ddpm_pert as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_PLAN = ["mcedm_ddpm_temb_row_count", "mcedm_ddpm_temb_rows", "mcedm_ddpm_workspace_bytes_t", "mcedm_ddpm_forward_t",
            "mcedm_ddpm_edm_denoise_t"]
NEW_OPS = ["mcedm_op_conv_bias_batch", "mcedm_op_conv_wino_sums_bias_batch"]
FAKE = 0x1000            # a non-null pointer no entry may dereference: every call below must fail on the host


def test_new_symbols_in_header_binding_and_library():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mcedm_hip.h")).read(), flags=re.S)
    nm = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    lib = L.load()
    for n in NEW_PLAN + NEW_OPS:
        assert re.search(rf"\bint {n}\s*\(", hdr), n
        assert re.search(rf"\bT {n}$", nm, flags=re.M), n
        getattr(lib, n)
    assert set(NEW_PLAN) <= set(L.EXPORTS) and set(NEW_OPS) <= set(L.OP_EXPORTS)
    assert lib.mcedm_version() == L.ABI_VERSION == 4
    for m in ("temb_rows", "forward_t", "edm_denoise_t", "workspace_bytes_t", "temb_row_count"):
        assert hasattr(L.DdpmPlan, m), m


def err(lib):
    return lib.mcedm_last_error().decode()


def plans():
    return {k: A.make_plan(L, A.ALL[k]) for k in ("one", "nrb2", "head_narrow3", "cat_one2")}


def test_row_count_is_the_sum_of_the_block_widths():
    for tag, cfg in A.ALL.items():
        want = sum(s[0] for n, s in A.ddo.param_shapes(cfg) if n.endswith(".temb_proj.weight"))
        assert A.make_plan(L, cfg).temb_row_count == want, tag
    assert A.make_plan(L, A.ALL["rows3"]).temb_row_count == 2816
    lib = L.load()
    assert lib.mcedm_ddpm_temb_row_count(None, C.byref(C.c_int32())) == -1 and "null" in err(lib)


def test_temb_rows_rejects_on_the_host():
    lib = L.load()
    p = plans()["one"]
    assert lib.mcedm_ddpm_temb_rows(p._h, FAKE, None, 2, FAKE, None) == -1 and "null" in err(lib)          # t
    assert lib.mcedm_ddpm_temb_rows(p._h, FAKE, FAKE, 2, None, None) == -1 and "null" in err(lib)          # rows_out
    assert lib.mcedm_ddpm_temb_rows(None, FAKE, FAKE, 2, FAKE, None) == -1
    for B in (0, -3, 65536):
        assert lib.mcedm_ddpm_temb_rows(p._h, FAKE, FAKE, B, FAKE, None) == -1 and "batch" in err(lib), B
    with pytest.raises(RuntimeError, match="1-D"):
        p.temb_rows(torch.empty(1, dtype=torch.uint8), torch.zeros(2, 2))
    with pytest.raises(RuntimeError, match="fp32"):
        p.temb_rows(torch.empty(1, dtype=torch.uint8), torch.zeros(2, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="device tensors"):
        p.temb_rows(torch.empty(1, dtype=torch.uint8), torch.zeros(2))


def test_forward_t_rejects_on_the_host():
    lib = L.load()
    P = plans()
    B = 2

    def call(plan, x=FAKE, sc=None, cmap=None, cat=None, t=FAKE, out=FAKE, ws=FAKE, nbytes=None, batch=B):
        nbytes = plan.workspace_bytes_t(B) if nbytes is None else nbytes
        return lib.mcedm_ddpm_forward_t(plan._h, FAKE, x, sc, cmap, cat, t, out, ws, nbytes, batch, None)

    for tag, plan in P.items():
        assert call(plan, t=None) == -1 and "null" in err(lib), tag
        assert call(plan, x=None) == -1 and call(plan, out=None) == -1 and call(plan, ws=None) == -1, tag
        for bad in (0, -1):
            assert call(plan, batch=bad) == -1 and "batch" in err(lib), (tag, bad)
        assert call(plan, nbytes=plan.workspace_bytes_t(B) - 1) == -3 and "ddpm_forward_t: workspace too small" in err(lib), tag
        assert plan.workspace_bytes_t(B) >= plan.workspace_bytes(B) + B * plan.temb_row_count * 4, tag
    # a conditioning pointer the plan has no use for
    assert call(P["one"], sc=FAKE) == -1 and "self-conditioning" in err(lib)
    assert call(P["cat_one2"], sc=FAKE) == -1 and "self-conditioning" in err(lib)
    for tag in ("one", "nrb2", "cat_one2"):
        assert call(P[tag], cmap=FAKE) == -1 and "cond_enc head" in err(lib), tag
    for tag in ("one", "nrb2", "head_narrow3"):
        assert call(P[tag], cat=FAKE) == -1 and "cat_cond" in err(lib), tag
    # the binding raises in Python before it calls
    pk = torch.empty(1, dtype=torch.uint8)
    x = torch.zeros(B, 2, 8, 8)
    with pytest.raises(RuntimeError, match=r"shape \[2\]"):
        P["one"].forward_t(pk, x, torch.zeros(3))
    with pytest.raises(RuntimeError, match="fp32"):
        P["one"].forward_t(pk, x, torch.zeros(B, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="cat_cond plan"):
        P["one"].forward_t(pk, x, torch.zeros(B), cond=torch.zeros(B, 2, 8, 8))
    with pytest.raises(RuntimeError, match="input"):
        P["one"].forward_t(pk, torch.zeros(B, 2, 16, 16), torch.zeros(B))


def test_edm_denoise_t_rejects_on_the_host():
    lib = L.load()
    P = plans()
    B = 2

    def call(plan, x=FAKE, cond=None, sigma=FAKE, sd=1.0, D=FAKE, ws=FAKE, nbytes=None, batch=B):
        nbytes = plan.workspace_bytes_t(B) if nbytes is None else nbytes
        return lib.mcedm_ddpm_edm_denoise_t(plan._h, FAKE, x, cond, sigma, sd, D, None, ws, nbytes, batch, None)

    cat = P["cat_one2"]
    assert call(cat, sigma=None) == -1 and "null" in err(lib)
    assert call(cat, x=None) == -1 and call(cat, D=None) == -1 and call(cat, ws=None) == -1
    for bad in (0, -1):
        assert call(cat, batch=bad) == -1 and "batch" in err(lib), bad
    assert call(cat, sd=0.0) == -1 and "sigma_data" in err(lib)
    assert call(cat, nbytes=cat.workspace_bytes_t(B) - 1) == -3 and "ddpm_edm_denoise_t: workspace too small" in err(lib)
    for tag in ("one", "nrb2", "head_narrow3"):
        assert call(P[tag], cond=FAKE) == -1 and "cat_cond" in err(lib), tag
    pk = torch.empty(1, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match=r"shape \[2\]"):
        cat.edm_denoise_t(pk, torch.zeros(B, 2, 8, 8), torch.zeros(1))
    with pytest.raises(RuntimeError, match="cond"):
        cat.edm_denoise_t(pk, torch.zeros(B, 2, 8, 8), torch.zeros(B), cond=torch.zeros(B, 3, 8, 8))


def test_conv_launchers_without_a_bias_row_per_sample_refuse_it():
    """Cout = 2 at 64 x 64 (the small-Cout kernel), the stride-2 conv, a 1 x 1 conv, an up-sampling 3 x 3 conv, and a row pitch
    below Cout: MCEDM_ERR_INVALID on the host, whatever kernel the dispatcher would have chosen."""
    lib = L._bind_ops()

    def call(Cout, k, resample, Hs, H, bias_batch, bias=FAKE):
        return lib.mcedm_op_conv_bias_batch(FAKE, None, 64, 0, None, 0, 0, resample, Hs, Hs, H, H, FAKE, bias, bias_batch, None, 0, FAKE,
                                            Cout, 3, k, None)

    for what, args in (("Cout 2", (2, 3, L.RS_NONE, 64, 64, 32)), ("stride 2", (64, 3, L.RS_S2, 32, 16, 64)),
                       ("1 x 1", (64, 1, L.RS_NONE, 16, 16, 64)), ("up-sampled", (64, 3, L.RS_UP, 8, 16, 64)),
                       ("pitch < Cout", (64, 3, L.RS_NONE, 16, 16, 32)), ("negative", (64, 3, L.RS_NONE, 16, 16, -64))):
        assert call(*args) == -1 and "bias" in err(lib), what
    assert call(64, 3, L.RS_NONE, 16, 16, 64, bias=None) == -1 and "bias" in err(lib)
    rc = lib.mcedm_op_conv_wino_sums_bias_batch(FAKE, None, 64, 0, None, 0, 0, 0, 8, 16, FAKE, None, 64, None, 0, FAKE, FAKE, 64, 3, None)
    assert rc == -1 and "bias_batch" in err(lib)


# what the six size queries returned before the per-sample entries existed (a build of the parent commit), per row of
# _ddpm_arch.ALL and B in (1, 2, 5): ddpm, repaint, ddim, ddpm_vp_sampler, ddpm_cond_ddim, ddpm_edm_sampler
QUERIES = ["mcedm_ddpm_workspace_bytes", "mcedm_repaint_workspace_bytes", "mcedm_ddim_workspace_bytes",
           "mcedm_ddpm_vp_sampler_workspace_bytes", "mcedm_ddpm_cond_ddim_workspace_bytes", "mcedm_ddpm_edm_sampler_workspace_bytes"]
WORKSPACE_BYTES = {
    "nrb2": [[668928, 687360, 677120, 752896, 744704, 689408], [1334528, 1371392, 1350912, 1502464, 1486080, 1375488], [3331328, 3423488, 3372288, 3751168, 3710208, 3433728]],
    "one": [[134656, 139264, 136704, 155648, 153600, 139776], [267776, 276992, 271872, 309760, 305664, 278016], [667136, 690176, 677376, 772096, 761856, 692736]],
    "r48": [[3642624, 3725568, 3679488, 4315392, 4278528, 3734784], [7282944, 7448832, 7356672, 8628480, 8554752, 7467264], [18203904, 18618624, 18388224, 21567744, 21383424, 18664704]],
    "wide0": [[2919424, 2993152, 2952192, 3255296, 3222528, 3001344], [5835776, 5983232, 5901312, 6507520, 6441984, 5999616], [14584832, 14953472, 14748672, 16264192, 16100352, 14994432]],
    "wide3": [[4263680, 4337408, 4296448, 4599552, 4566784, 4345600], [8523520, 8670976, 8589056, 9195264, 9129728, 8687360], [21303040, 21671680, 21466880, 22982400, 22818560, 21712640]],
    "narrow": [[249856, 268288, 258048, 301056, 292864, 270336], [497664, 534528, 514048, 600064, 583680, 538624], [1241088, 1333248, 1282048, 1497088, 1456128, 1343488]],
    "deep": [[1128960, 1202688, 1161728, 1333760, 1300992, 1210880], [2251264, 2398720, 2316800, 2660864, 2595328, 2415104], [5618176, 5986816, 5782016, 6642176, 6478336, 6027776]],
    "rows3": [[879872, 898304, 888064, 963840, 955648, 900352], [1748224, 1785088, 1764608, 1916160, 1899776, 1789184], [4353280, 4445440, 4394240, 4773120, 4732160, 4455680]],
    "head_narrow3": [[249856, 268288, 258048, 301056, 292864, 270336], [497664, 534528, 514048, 600064, 583680, 538624], [1241088, 1333248, 1282048, 1497088, 1456128, 1343488]],
    "head_r48": [[3642624, 3725568, 3679488, 4315392, 4278528, 3734784], [7282944, 7448832, 7356672, 8628480, 8554752, 7467264], [18203904, 18618624, 18388224, 21567744, 21383424, 18664704]],
    "cat_one2": [[135168, 139776, 137216, 156160, 154112, 140288], [268800, 278016, 272896, 310784, 306688, 279040], [669696, 692736, 679936, 774656, 764416, 695296]],
    "cat_narrow1": [[251904, 270336, 260096, 303104, 294912, 272384], [501760, 538624, 518144, 604160, 587776, 542720], [1251328, 1343488, 1292288, 1507328, 1466368, 1353728]],
}


@pytest.mark.parametrize("tag", list(A.ALL))
def test_existing_size_queries_are_unchanged(tag):
    assert set(WORKSPACE_BYTES) == set(A.ALL)
    plan = A.make_plan(L, A.ALL[tag])
    for row, B in zip(WORKSPACE_BYTES[tag], (1, 2, 5)):
        got = [plan._bytes(q, q, B) for q in QUERIES]
        assert got == row, (tag, B, got)
        # the new query: the network's bytes behind the table, conv_in's rows and the labels, each 256-byte aligned
        up = lambda n: (n + 255) // 256 * 256
        in_total = A.ALL[tag].in_channels * (2 if A.ALL[tag].self_cond else 1) + (A.ALL[tag].cond_channels if A.ALL[tag].cat_cond else 0)
        assert plan.workspace_bytes_t(B) == row[0] + up(B * plan.temb_row_count * 4) + up(B * in_total * 16) + up(B * 4), (tag, B)


@pytest.mark.parametrize("tag", list(A.ALL))
def test_fp32_oracle_reproduces_the_golden(golden, tag):
    """ddpm_oracle.model_forward with t of shape [B] at (3, 937), fp32, against the reference's stored output at the bar (the
    generator asserted bit equality at its own thread count)."""
    g = golden("ddpm_pert.npz")
    ts = T.T_PAIRS[0]
    r = A.bar_ratio(T.oracle_forward(tag, A.params(tag), ts), g[T.key(tag, ts)])
    assert r <= 1.0, (tag, r)
    assert T.key(tag, T.T_PAIRS[1]) in g


def test_model_forward_takes_one_t_or_one_per_sample():
    """Model.forward: any other length of t raises ValueError (before anything touches the device)."""
    from mcedm_amd.ddim_blocks import Model
    from tests import _ddpm_edm as D
    from tests.test_hip_module import wrap
    net = Model(wrap(D.hparams_dict()))
    x = torch.zeros(4, D.CFG.in_channels, D.CFG.resolution, D.CFG.resolution)
    with torch.no_grad(), pytest.raises(ValueError, match="one per sample"):
        net(x, torch.zeros(3))


@pytest.mark.parametrize("kind", list(T.STEP_CASES))
def test_fp64_loss_formula_agrees_with_the_stored_values(golden, kind):
    """tests/_ddpm_pert.step_forward64 (the formula the GPU test's bound refers to) against what the generator stored: the fp64
    loss to fp64 rounding, the reference's own fp32 outputs at the bar, its fp32 loss within a quarter of rtol 1e-5."""
    g = golden("ddpm_pert_steps.npz")
    P64 = T.step_params(kind, torch.float64)
    for case in T.STEP_CASES[kind]:
        key = f"{kind}::{case}"
        out, x0, loss = T.step_forward64(kind, case, P64)
        assert abs(float(loss) - float(g[f"{key}::loss64"])) <= 1e-12 * abs(float(loss)), key
        assert A.bar_ratio(g[f"{key}::output"], out) <= 1.0 and A.bar_ratio(g[f"{key}::x0_t"], x0) <= 1.0, key
        assert abs(float(g[f"{key}::loss"]) - float(loss)) <= 0.25e-5 * abs(float(loss)) and float(g[f"{key}::loss_bar"]) == 1e-5, key
