"""CPU-only checks of the C ABI (no compute calls): libmcedm_hip.so loads without a GPU, exports exactly the symbols
include/mcedm_hip.h declares, and its host-side entry points (plan construction, parameter table, sizes, the sigma
schedule, argument validation) behave as documented."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import pytest
import torch

import mcedm_amd  # noqa: F401
from mcedm_amd import abi
from mcedm_amd import lib as L
from oracle import mcedm_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mcedm_hip.h")


def declared_symbols(with_args=False):
    """The names the header declares (or name -> argument text), by a regex of this file's own: independent of mcedm_amd.abi."""
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    if with_args:
        return dict(re.findall(r"\b(mcedm_[a-z0-9_]+)\s*\(([^)]*)\)", src))
    return sorted(set(re.findall(r"\b(mcedm_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    lib = L.load()
    names = declared_symbols()
    assert len(names) >= 36
    assert set(abi.PROTOS) == set(names), set(abi.PROTOS) ^ set(names)
    for n, args in declared_symbols(with_args=True).items():
        fn = getattr(lib, n)                             # AttributeError == header / library drift
        void = args.strip() == "void"
        assert fn.argtypes or void, n                    # bound, with its argument types
        assert len(fn.argtypes) == (0 if void else args.count(",") + 1), n
    assert len(declared_symbols(with_args=True)) == len(names)
    nm = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = sorted(set(re.findall(r"\bT (mcedm_[a-z0-9_]+)$", nm, flags=re.M)))
    assert exported == names, (set(exported) ^ set(names))
    assert sorted(set(L.EXPORTS + L.OP_EXPORTS)) == names, set(L.EXPORTS + L.OP_EXPORTS) ^ set(names)
    assert lib.mcedm_version() == 4
    # the header's constants the binding mirrors
    hdr = open(HEADER).read()
    consts = {k: int(v) for k, v in re.findall(r"#define (MCEDM_[A-Z0-9_]+) (\d+)\b", hdr)}
    assert consts["MCEDM_ABI_VERSION"] == L.ABI_VERSION == 4
    assert consts["MCEDM_GN_SYNC_WORDS"] == L.GN_SYNC_WORDS
    for name, idx in L.VARIANTS.items():
        assert consts["MCEDM_VARIANT_" + name.upper()] == idx, name


# The C spelling of each scalar class, this file's own (size_t and uint64_t are one class to ctypes and one type to the compiler on
# LP64).  A scalar that mcedm_amd.abi misread is spelled wrongly below, and the compiler refuses it.
_C_SCALAR = {C.c_int: "int", C.c_int64: "int64_t", C.c_uint64: "uint64_t", C.c_float: "float", C.c_double: "double"}


def _c_type(ctype, text):
    """How the generated C spells one parsed type: a scalar by its ctypes class, a pointer as abi.DECLS gives it."""
    if ctype is None:
        return "void"
    if ctype in _C_SCALAR:
        return _C_SCALAR[ctype]
    assert "*" in text or "[" in text, (ctype, text)
    if ctype not in (C.c_void_p, C.c_char_p):            # POINTER(struct): the struct the header names
        assert text == f"const {ctype._type_.__name__}*" and abi.STRUCTS[ctype._type_.__name__] is ctype._type_, text
    else:
        assert (ctype is C.c_char_p) == (text.replace("const ", "") == "char*"), text
    return text


def _prototypes_c(protos):
    lines = ['#include "mcedm_hip.h"']
    for n, (ret, args) in protos.items():
        rtext, atexts = abi.DECLS[n]
        assert len(args) == len(atexts), n
        lines.append(f"{_c_type(ret, rtext)} (*p_{n})({', '.join(map(_c_type, args, atexts)) or 'void'}) = &{n};")
    return "\n".join(lines) + "\n"


def test_parsed_abi_agrees_with_a_c_compiler(tmp_path):
    """What mcedm_amd.abi read from the header, handed back to a C compiler next to the header itself.  Every prototype: its address
    initialises a function pointer whose type is spelled from abi.PROTOS (compiled, not linked), so a miscounted or misread argument
    or return type is an incompatible-pointer error.  Every struct: sizeof, each field's offset and a pointer of the parsed type to
    each field, against the ctypes classes."""
    cc = next(filter(None, map(shutil.which, ("cc", os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang")))), None)
    assert cc, "no C compiler found (cc, or ROCm's clang): m-cedm_amd/build.py needs one as well"

    def compile_c(name, text, *flags):
        (tmp_path / name).write_text(text)
        return subprocess.run([cc, "-std=c11", "-I" + os.path.dirname(HEADER), "-Werror=incompatible-pointer-types", "-Werror=int-conversion",
                               *flags, name], cwd=tmp_path, capture_output=True, text=True)

    r = compile_c("protos.c", _prototypes_c(abi.PROTOS), "-c")
    assert r.returncode == 0, r.stderr[-3000:]
    # the check has teeth: size_t read as int, and double read as float, are refused
    ret, args = abi.PROTOS["mcedm_sqnorm"]
    assert args[1] is C.c_size_t
    assert compile_c("bad0.c", _prototypes_c({"mcedm_sqnorm": (ret, [args[0], C.c_int] + args[2:])}), "-c").returncode != 0
    ret, args = abi.PROTOS["mcedm_edm_denoise"]
    assert args[-2] is C.c_double
    assert compile_c("bad1.c", _prototypes_c({"mcedm_edm_denoise": (ret, args[:-2] + [C.c_float, args[-1]])}), "-c").returncode != 0

    assert len(abi.STRUCTS) == 10
    lines, want = ["#include <stdio.h>", '#include "mcedm_hip.h"', "int main(void) {"], {}
    for s, cls in abi.STRUCTS.items():
        lines += [f"  static {s} v_{s};", f'  printf("{s} %zu\\n", sizeof({s}));']
        want[s] = C.sizeof(cls)
        for f, t in cls._fields_:
            if hasattr(t, "_length_"):
                spelled = f"{_C_SCALAR[t._type_]} (*q)[{t._length_}]"
            elif t in _C_SCALAR:
                spelled = f"{_C_SCALAR[t]} *q"
            else:                                        # (every pointer field of the header points at const)
                spelled = f"const {_C_SCALAR[t._type_]} **q"
            lines += [f'  printf("{s}.{f} %zu\\n", offsetof({s}, {f}));', f"  {{ {spelled} = &v_{s}.{f}; (void)q; }}"]
            want[f"{s}.{f}"] = getattr(cls, f).offset
    r = compile_c("sizes.c", "\n".join(lines + ["  return 0;", "}"]) + "\n", "-o", "sizes")
    assert r.returncode == 0, r.stderr[-3000:]
    out = subprocess.run([str(tmp_path / "sizes")], capture_output=True, text=True, check=True).stdout
    assert {k: int(v) for k, v in (line.split() for line in out.splitlines())} == want


@pytest.mark.parametrize("line,text", [(3, "typedef union { int a; float b; } mcedm_u;"), (2, "#define MCEDM_TWICE(x) (2 * (x))"),
                                       (3, "int mcedm_f(unsigned int flags);"), (3, "int mcedm_g(int (*callback)(void));"),
                                       (4, "}")])
def test_header_parser_refuses_what_it_does_not_know(tmp_path, line, text):
    """A construct outside the header's own grammar is an error that names the file and line, never skipped: a by-value type with no
    ctypes class here, a union, a function-like macro, a callback, a stray brace.  MCEDM_HEADER selects the header read."""
    hdr = tmp_path / "other.h"
    hdr.write_text("\n" * (line - 1) + text + "\n")
    r = subprocess.run([sys.executable, abi.__file__], env=dict(os.environ, MCEDM_HEADER=str(hdr)), capture_output=True, text=True)
    assert r.returncode != 0 and f"ValueError: {hdr}:{line}: " in r.stderr, r.stderr[-2000:]


def test_plan_parameter_table_matches_state_dict_order():
    for cfg in (orc.UNetConfig(), orc.UNetConfig(ch=128, ch_mult=(1, 1, 1, 1), attn_resolutions=(16,))):
        plan = L.Plan(cfg.in_channels, cfg.cond_channels, cfg.out_ch, cfg.ch, cfg.ch_mult, cfg.num_res_blocks,
                      cfg.attn_resolutions, cfg.resolution)
        ref = orc.param_shapes(cfg)
        assert plan.param_names == [n for n, _ in ref]
        assert plan.param_shapes == [tuple(s) for _, s in ref]
        assert plan.packed_bytes > 4 * sum(int(torch.tensor(s).prod()) for _, s in ref)
        assert plan.workspace_bytes(2, 32, 32) < plan.workspace_bytes(2, 32, 32, training=True)
        assert plan.sampler_workspace_bytes(2, 32, 32) > plan.workspace_bytes(2, 32, 32)


def test_dx_cond_plans_list_the_head_parameters_in_state_dict_order():
    """dx_cond (adm_blocks.py:233-280): cat_dx widens conv_in; dx_enc / combine_enc are registered before self.enc."""
    import dataclasses
    for mode, code in (("cat", L.DX_CAT), ("enc", L.DX_ENC)):
        cfg = dataclasses.replace(orc.UNetConfig(in_channels=1, cond_channels=1, out_ch=1), dx_channels=1, dx_mode=mode)
        plan = L.Plan(cfg.in_channels, cfg.cond_channels, cfg.out_ch, cfg.ch, cfg.ch_mult, cfg.num_res_blocks,
                      cfg.attn_resolutions, cfg.resolution, dx_channels=1, dx_mode=code)
        ref = orc.param_shapes(cfg)
        assert plan.param_names == [n for n, _ in ref] and plan.param_shapes == [tuple(s) for _, s in ref]
    assert plan.param_names[4:10] == ["dx_enc.0.weight", "dx_enc.0.bias", "dx_enc.2.weight", "dx_enc.2.bias",
                                      "combine_enc.weight", "combine_enc.bias"]
    with pytest.raises(RuntimeError, match="dx_channels"):
        L.Plan(1, 1, 1, 64, (1, 1, 1), 1, (32,), 128, dx_channels=1, dx_mode=L.DX_NONE)


def test_t_steps_host_helper_matches_oracle():
    sd = L.sampler_desc(orc.SamplerParams(timesteps=18))
    t = torch.tensor(L.edm_t_steps(sd), dtype=torch.float64)
    torch.testing.assert_close(t, orc.edm_t_steps(18, 0.002, 80.0, 7.0), rtol=1e-14, atol=0)
    assert t[-1] == 0 and t[0] == 80.0


@pytest.mark.parametrize("ch,mult,attn", [(96, (1, 1), ()), (32, (1, 5), ()), (64, (1, 1, 1), (64,)), (160, (1,), ())])
def test_attention_width_not_a_multiple_of_64_is_rejected(ch, mult, attn):
    """head_dim = C / (C // 64) in the reference (adm_blocks.py:135,175); only head_dim 64 is built, so a
    width like 96 or 160 at an attention block must be refused, not computed with 64-wide heads."""
    width_bad = any((ch * m) % 64 and ch * m >= 64 for lv, m in enumerate(mult) if lv == len(mult) - 1 or (128 >> lv) in attn)
    if width_bad:
        with pytest.raises(RuntimeError, match="channels_per_head"):
            L.Plan(2, 2, 2, ch, mult, 1, attn, 128)
    else:
        L.Plan(2, 2, 2, ch, mult, 1, attn, 128)


@pytest.mark.parametrize("ch,mult,name,C", [(48, (2, 1), "dec.8x8_block1.norm0", 144), (72, (2, 8), "enc.16x16_block0.norm0", 144)])
def test_groupnorm_width_its_groups_do_not_divide_is_rejected(ch, mult, name, C):
    """GroupNorm(C) has min(32, C / 4) groups (adm_blocks.py:89): a level width or a concat of 128 channels or more that is not a
    multiple of 32 (144 = 96 + 48; a 144-wide level) has no GroupNorm in the reference either; plan_create names the first such
    norm instead of leaving it to the first forward.  The neighbours the kernels do serve -- 120 = 80 + 40 (30 groups), 160 =
    80 + 80, 72 = 48 + 24 -- still build."""
    with pytest.raises(RuntimeError, match=rf"GroupNorm {name} has {C} channels, not a multiple of its 32 groups"):
        L.Plan(2, 2, 2, ch, mult, 1, (), 16)
    L.Plan(2, 2, 2, 40, (2, 1), 1, (), 16)
    L.Plan(1, 0, 3, 24, (1, 2, 2), 1, (), 16)


def test_host_side_argument_validation():
    with pytest.raises(RuntimeError, match="multiple of 8"):
        L.Plan(2, 2, 2, 12, (1,), 1, (), 128)
    plan = L.Plan(2, 2, 2, 64, (1, 1, 1), 1, (32,), 128)
    with pytest.raises(RuntimeError, match="multiples of 4"):
        plan.workspace_bytes(1, 30, 32)
    sd = L.sampler_desc(orc.SamplerParams(timesteps=1))
    with pytest.raises(RuntimeError, match="timesteps"):
        L.edm_t_steps(sd)
    with pytest.raises(RuntimeError, match="CPU tensor"):
        plan.forward(torch.zeros(8), torch.zeros(1, 2, 32, 32), torch.zeros(1))


def _last():
    return L.load().mcedm_last_error().decode()


def _up(nbytes):
    return (nbytes + 255) // 256 * 256


def test_host_side_rejections_of_the_adm_entries():
    """mcedm_unet_forward(_dx), mcedm_edm_denoise(_dx), the Heun samplers (plain, _rng, _guided, _dxcond), mcedm_vp_heun_sample,
    mcedm_cond_ddim_sample, mcedm_edm_denoise_backward(_dx), mcedm_unet_backward and the four size queries: the return code and
    the exact text for a null plan / packed / workspace, B = 0, H off the plan's grid, n_noise neither 1 nor B, a workspace one
    byte short (both byte counts named; the backward's include its scratch), dx on a plan without dx_cond, and which check speaks
    when two fail at once.  All on the host, before any launch: the dummy pointers are never dereferenced.

    The bytes an entry needs come from the size queries alone.  A query lays the network out with n_noise = B, the samplers with
    one label for the batch, as mcedm_cond_ddim_workspace_bytes does: what that query reports minus the DDIM sampler's own six
    buffers is the network at n_noise = 1, and a sampler's query minus mcedm_unet_workspace_bytes is that sampler's own buffers."""
    from types import SimpleNamespace
    lib = L.load()
    mk = lambda c, **kw: L.Plan(c, c, c, 64, (1, 1, 1), 1, (32,), 128, **kw)      # noqa: E731
    joint, single, dxp = mk(2), mk(1), mk(1, dx_channels=1, dx_mode=L.DX_ENC)
    one = C.c_void_p(4096)
    B, H, W = 3, 32, 32
    vpp = C.POINTER(C.c_void_p)
    ptrs = lambda p: C.cast((C.c_void_p * len(p.param_names))(*[4096] * len(p.param_names)), vpp)      # noqa: E731
    mk_sd = lambda N: L.sampler_desc(orc.SamplerParams(timesteps=N))      # noqa: E731
    gd = L.GuidanceDesc(1, 0.002, 0.03125, 0.0, 0.0, 1.0, 0.0, 1.0, 5.0)
    def mk_vd(N, cc):             # two steps' tables, of which the sampler is told to walk N
        d = L.vp_sampler_desc(2, cc, [5.0, 1.0, 0.0], [5.0, 1.0], [900.0, 800.0, 700.0, 0.0], 1.0, 0.0)
        d.timesteps = N
        return d
    ae = torch.linspace(1.0, 0.1, 11)
    mk_cd = lambda N, cc: L.cond_ddim_desc(SimpleNamespace(timesteps=N, skip_type="uniform", eta=0.0, w=0.0), ae, cc, False)      # noqa: E731

    def net_bytes(p, n):          # header + activations of the inference layout with n noise labels
        if n == B:
            return p.workspace_bytes(B, H, W)
        hw4 = H * W * 4
        own = 2 * _up(B * p.in_channels * hw4) + 2 * _up(B * p.out_channels * hw4) + 2 * _up(B * p.cond_channels * hw4)
        return p.cond_ddim_workspace_bytes(B, H, W) - own

    for p in (joint, single, dxp):
        state = B * p.in_channels * H * W
        heun = 3 * _up(state * 8) + 2 * _up(state * 4)
        assert net_bytes(p, 1) < net_bytes(p, B)
        assert p.sampler_workspace_bytes(B, H, W) - p.workspace_bytes(B, H, W) == heun + 3 * _up(state * 4)
        assert p.vp_sampler_workspace_bytes(B, H, W) - p.workspace_bytes(B, H, W) == heun + _up(B * p.cond_channels * H * W * 4)

    def own_bytes(p, query):
        return getattr(p, query)(B, H, W) - p.workspace_bytes(B, H, W)

    # name -> (who in the shared texts, text of a null plan, plan, bytes needed with n labels, call(plan, packed, workspace, bytes, B, H, n))
    guided_text = ("heun_sample_guided: PDE guidance is defined for the single-task sampler (state u, conditioning h in cond[:, 0]; "
                   "mask NULL), models/ddim.py:1532-1601; the joint model's hook fails in the reference (models/mcedm.py:500-518)")
    dxcond_text = ("heun_sample_dxcond: needs a dx_cond plan of the single-task model (state u, conditioning h in cond[:, 0], one dx "
                   "channel), models/ddim.py:1424-1450, 1532-1601")
    sd, vd2, vd1, cd2, cd1 = mk_sd(3), mk_vd(2, 2), mk_vd(2, 1), mk_cd(3, 2), mk_cd(3, 1)
    heun_need = lambda p: lambda n: own_bytes(p, "sampler_workspace_bytes") + net_bytes(p, 1)      # noqa: E731
    entries = {
        "unet_forward": ("unet_forward", None, joint, lambda n: net_bytes(joint, n), lambda p, pk, ws, nb, b, h, n:
                         lib.mcedm_unet_forward(p, pk, one, one, None, one, n, one, ws, nb, b, h, W, 0, None)),
        "unet_forward_dx": ("unet_forward", None, dxp, lambda n: net_bytes(dxp, n), lambda p, pk, ws, nb, b, h, n:
                            lib.mcedm_unet_forward_dx(p, pk, one, one, one, one, one, n, one, ws, nb, b, h, W, 0, None)),
        "edm_denoise": ("edm_denoise", None, joint, lambda n: net_bytes(joint, n), lambda p, pk, ws, nb, b, h, n:
                        lib.mcedm_edm_denoise(p, pk, one, one, n, one, one, None, ws, nb, b, h, W, 0, 0.5, None)),
        "edm_denoise_dx": ("edm_denoise", None, dxp, lambda n: net_bytes(dxp, n), lambda p, pk, ws, nb, b, h, n:
                           lib.mcedm_edm_denoise_dx(p, pk, one, one, one, n, one, one, None, ws, nb, b, h, W, 0, 0.5, None)),
        "heun_sample": ("heun_sample", None, joint, heun_need(joint), lambda p, pk, ws, nb, b, h, n, d=sd:
                        lib.mcedm_heun_sample(p, pk, C.byref(d), one, one, one, one, one, 1, ws, nb, b, h, W, None)),
        "heun_sample_rng": ("heun_sample", None, joint, heun_need(joint), lambda p, pk, ws, nb, b, h, n, d=sd:
                            lib.mcedm_heun_sample_rng(p, pk, C.byref(d), one, one, one, one, one, 1, ws, nb, b, h, W, None)),
        "heun_sample_guided": ("heun_sample", guided_text, single, heun_need(single), lambda p, pk, ws, nb, b, h, n, d=sd:
                               lib.mcedm_heun_sample_guided(p, pk, C.byref(d), C.byref(gd), one, None, one, one, one, 1, ws, nb, b,
                                                            h, W, None)),
        "heun_sample_dxcond": ("heun_sample", dxcond_text, dxp, heun_need(dxp), lambda p, pk, ws, nb, b, h, n, d=sd:
                               lib.mcedm_heun_sample_dxcond(p, pk, C.byref(d), C.byref(gd), None, one, one, one, one, 1, ws, nb, b,
                                                            h, W, None)),
        "vp_heun_sample": ("vp_heun_sample", None, joint, lambda n: own_bytes(joint, "vp_sampler_workspace_bytes") + net_bytes(joint, 1),
                           lambda p, pk, ws, nb, b, h, n, d=vd2:
                           lib.mcedm_vp_heun_sample(p, pk, C.byref(d), one, one, None, one, 1, ws, nb, b, h, W, None)),
        "cond_ddim_sample": ("cond_ddim_sample", None, joint, lambda n: joint.cond_ddim_workspace_bytes(B, H, W),
                             lambda p, pk, ws, nb, b, h, n, d=cd2:
                             lib.mcedm_cond_ddim_sample(p, pk, C.byref(d), one, one, None, one, one, 1, ws, nb, b, h, W, None)),
        "edm_denoise_backward": ("denoise_backward", None, joint, lambda n: joint.workspace_bytes(B, H, W, True),
                                 lambda p, pk, ws, nb, b, h, n, g=ptrs(joint):
                                 lib.mcedm_edm_denoise_backward(p, pk, g, one, one, n, one, one, g, ws, nb, b, h, W, 0.5, None)),
        "unet_backward": ("denoise_backward", None, joint, lambda n: joint.workspace_bytes(B, H, W, True),
                          lambda p, pk, ws, nb, b, h, n, g=ptrs(joint):
                          lib.mcedm_unet_backward(p, pk, g, one, one, None, one, n, one, g, ws, nb, b, h, W, None)),
    }
    samplers = [k for k in entries if "sample" in k]
    for name, (who, null_plan, plan, need_of, call) in entries.items():
        need = need_of(B)
        assert call(None, one, one, need, B, H, B) == -1 and _last() == (null_plan or f"{who}: null argument"), name
        for args in ((plan._h, None, one), (plan._h, one, None)):
            assert call(*args, need, B, H, B) == -1 and _last() == f"{who}: null argument", (name, args)
        assert call(plan._h, one, one, need, 0, H, 0) == -1 and _last() == f"layout: empty shape B=0 H={H} W={W}", name
        assert call(plan._h, one, one, need, B, 30, B) == -1, name
        assert _last() == f"layout: H=30 W={W} must be multiples of 4 (2^(levels-1))", name
        for n in ((B,) if name in samplers or "backward" in name else (B, 1)):
            need = need_of(n)
            assert call(plan._h, one, one, need - 1, B, H, n) == -3, (name, n)
            assert _last() == f"{who}: workspace too small ({need - 1} < {need} bytes)", (name, n)
        if name not in samplers:        # (the samplers take no n_noise: one label for the batch)
            assert call(plan._h, one, one, need, B, H, 2) == -1 and _last() == f"layout: n_noise=2 must be 1 or B={B}", name
            # two at once: the shape speaks before n_noise, and both before the workspace
            assert call(plan._h, one, one, 0, B, 30, 2) == -1 and "must be multiples of 4" in _last(), name
            assert call(plan._h, one, one, 0, B, H, 2) == -1 and "n_noise=2 must be 1 or B=3" in _last(), name
        assert call(plan._h, one, one, 0, 0, H, 0) == -1 and _last() == f"layout: empty shape B=0 H={H} W={W}", name
    # the backward's bytes include its scratch behind the training-mode activations
    assert joint.workspace_bytes(B, H, W, True) > joint.workspace_bytes(B, H, W)
    # dx given to a plan without dx_cond: it speaks before the layout and the workspace
    g = ptrs(single)
    for who, call in (("unet_forward", lambda b, nb: lib.mcedm_unet_forward_dx(single._h, one, one, one, one, None, one, b, one, one,
                                                                                nb, b, H, W, 0, None)),
                      ("edm_denoise", lambda b, nb: lib.mcedm_edm_denoise_dx(single._h, one, one, one, one, b, one, one, None, one, nb, b,
                                                                             H, W, 0, 0.5, None)),
                      ("denoise_backward", lambda b, nb: lib.mcedm_edm_denoise_backward_dx(single._h, one, g, one, one, one, b, one, one,
                                                                                           g, one, nb, b, H, W, 0.5, 0, None, None, None))):
        for b, nb in ((B, 1 << 30), (0, 0)):
            assert call(b, nb) == -1 and _last() == f"{who}: dx given to a plan without dx_cond", (who, b)
    # two at once on the samplers: a bad schedule speaks before a zero-byte workspace.  The EDM schedule divides by timesteps - 1,
    # so 1 is bad there; the VP and DDIM schedules hold from 1 step on (there the workspace speaks) and are bad at 0.
    for name in ("heun_sample", "heun_sample_rng", "heun_sample_guided", "heun_sample_dxcond"):
        plan, call = entries[name][2], entries[name][4]
        assert call(plan._h, one, one, 0, B, H, B, mk_sd(1)) == -1 and _last() == "heun_sample: timesteps=1 out of range", name
    plan, call = entries["vp_heun_sample"][2], entries["vp_heun_sample"][4]
    assert call(plan._h, one, one, 0, B, H, B, mk_vd(1, 2)) == -3 and _last().startswith("vp_heun_sample: workspace too small (0 < ")
    assert call(plan._h, one, one, 0, B, H, B, mk_vd(0, 2)) == -1 and _last() == "vp_heun_sample: timesteps=0 out of range"
    assert call(plan._h, one, one, 0, B, H, B, vd1) == -3          # fewer conditioning channels than the plan's: a staged cond'
    call = entries["cond_ddim_sample"][4]
    assert call(plan._h, one, one, 0, B, H, B, mk_cd(1, 2)) == -3 and _last().startswith("cond_ddim_sample: workspace too small (0 < ")
    assert call(plan._h, one, one, 0, B, H, B, mk_cd(0, 2)) == -1 and _last() == "cond_ddim_sample: bad schedule (timesteps=0 of 10)"
    assert call(plan._h, one, one, 0, B, H, B, cd1) == -3
    # the size queries
    sz = C.c_size_t()
    for q, extra in (("workspace_bytes", (0,)), ("workspace_bytes", (1,)), ("sampler_workspace_bytes", ()),
                     ("vp_sampler_workspace_bytes", ()), ("cond_ddim_workspace_bytes", ())):
        fn = getattr(lib, "mcedm_unet_workspace_bytes" if q == "workspace_bytes" else "mcedm_" + q)
        for pl in (joint, dxp):
            assert fn(None, B, H, W, *extra, C.byref(sz)) == -1 and _last() == f"{q}: null argument", q
            assert fn(pl._h, B, H, W, *extra, None) == -1 and _last() == f"{q}: null argument", q
            assert fn(pl._h, 0, H, W, *extra, C.byref(sz)) == -1 and _last() == f"layout: empty shape B=0 H={H} W={W}", q
            assert fn(pl._h, B, 30, W, *extra, C.byref(sz)) == -1, q
            assert _last() == f"layout: H=30 W={W} must be multiples of 4 (2^(levels-1))", q
            assert fn(pl._h, B, H, W, *extra, C.byref(sz)) == 0 and sz.value > 0, q


def test_dx_entry_points_validate_before_any_launch():
    """The dx_cond entry points reject a dx tensor / a dx-conditioned sampler on a plan built without dx_cond, and a wrong
    dx shape, on the host (no GPU in this container: the checks run before anything is enqueued)."""
    import ctypes as C
    lib = L.load()
    plain = L.Plan(1, 1, 1, 64, (1, 1, 1), 1, (32,), 128)
    x = torch.zeros(1, 1, 32, 32)
    with pytest.raises(RuntimeError, match="without dx_cond"):
        plain.denoise(torch.zeros(8), x, torch.ones(1), cond=x, dx=x)
    dxp = L.Plan(1, 1, 1, 64, (1, 1, 1), 1, (32,), 128, dx_channels=1, dx_mode=L.DX_ENC)
    with pytest.raises(RuntimeError, match=r"dx must be fp32 \[B, 1, H, W\]"):
        dxp.denoise(torch.zeros(8), x, torch.ones(1), cond=x, dx=torch.zeros(1, 2, 32, 32))
    sd = L.sampler_desc(orc.SamplerParams(timesteps=18))
    gd = L.GuidanceDesc(1, 0.002, 0.03125, 0.0, 0.0, 1.0, 0.0, 1.0, 5.0)
    one = C.c_void_p(16)          # never dereferenced: the plan check comes first
    rc = lib.mcedm_heun_sample_dxcond(plain._h, one, C.byref(sd), C.byref(gd), None, one, one, None, one, 1, one, 1 << 30, 1, 32, 32, None)
    assert rc == -1 and b"dx_cond plan" in lib.mcedm_last_error()
    assert dxp.workspace_bytes(2, 32, 32) > plain.workspace_bytes(2, 32, 32)      # the head's tensors are in the layout


def test_repaint_schedule_and_ddpm_plan_host_side():
    """f1 host pieces: the DDPM parameter table in Model.state_dict() order and the rounded sigma schedule
    (round_sigma of models/ddim.py:949-957 restated as an exact nearest-neighbour search) against the oracle's torch.cdist."""
    from oracle import ddpm_oracle as dorc
    from oracle import fixtures as fx
    cfg = dorc.DdpmConfig()                      # configs/model/ddim_res32.yaml: resolution 128, attention at 32
    plan = L.DdpmPlan(cfg.in_channels, cfg.out_ch, cfg.ch, cfg.ch_mult, cfg.num_res_blocks, cfg.attn_resolutions, cfg.resolution)
    ref = dorc.param_shapes(cfg)
    assert plan.param_names == [n for n, _ in ref] and plan.param_shapes == [tuple(s) for _, s in ref]
    assert plan.repaint_workspace_bytes(2) > plan.workspace_bytes(2) > 0
    betas = dorc.betas_of(cfg)
    steps, aext = dorc.edm_steps_of(betas), dorc.alphas_ext_of(betas)
    for N, churn in ((18, 0.0), (50, 15.0), (5, 0.0)):
        sp = dorc.RepaintParams(timesteps=N, S_churn=churn)
        rd, keep = L.repaint_desc(sp, steps, aext, 1, 1)
        t = torch.tensor(L.repaint_schedule(rd), dtype=torch.float64)
        smin, smax = max(sp.sigma_min, float(steps[-1])), min(sp.sigma_max, float(steps[0]))
        idx = torch.arange(N, dtype=torch.float64)
        ts = (smax ** (1 / sp.rho) + idx / (N - 1) * (smin ** (1 / sp.rho) - smax ** (1 / sp.rho))) ** sp.rho
        want = torch.cat([dorc.round_sigma(steps, ts), torch.zeros(1, dtype=torch.float64)])
        assert torch.equal(t, want), (N, (t - want).abs().max())
    with pytest.raises(RuntimeError, match="only 64 is built"):
        L.DdpmPlan(2, 2, 64, (1, 2), 1, (), 32)
    with pytest.raises(RuntimeError, match="multiple of 32"):
        L.DdpmPlan(2, 2, 48, (1,), 1, (), 32)


def test_ddim_timestep_sequence_equals_numpy_linspace():
    """the quad sequence is [int(s) for s in np.linspace(0, sqrt(0.8 n), N) ** 2] (models/ddim.py:826-828).
    numpy computes arange(N) * (stop / (N - 1)) and pins the last sample to stop; hi * i / (N - 1) truncates to a different
    timestep for 85 of ~1200 (n, N) pairs (n = 1000, N = 100: 799 instead of 800).  Host helper vs numpy on a sweep."""
    import numpy as np
    bad = []
    for n in (100, 250, 500, 1000, 2000, 4000):
        for N in list(range(1, 260)) + [n]:
            if N > n:
                continue
            ref = [int(s) for s in list(np.linspace(0, np.sqrt(n * 0.8), N) ** 2)]
            got = L.ddim_timesteps(n, N, "quad")
            if got != ref:
                bad.append((n, N))
            assert L.ddim_timesteps(n, N, "uniform") == list(range(0, n, n // N))
    assert not bad, bad[:10]
    assert L.ddim_timesteps(1000, 100, "quad")[-1] == 800 and L.ddim_timesteps(1000, 16, "quad")[1:4] == [3, 14, 31]
    with pytest.raises(RuntimeError, match="bad schedule"):
        L.ddim_timesteps(10, 11, "quad")


def test_bench_roofline_helpers():
    """bench.py's host-side arithmetic (no GPU): both roofline fractions of SURVEY.md 8(d) per forward and per state, and the
    HBM-bound kernel rows."""
    import bench
    f = bench.fractions("s128", 76.0, 12.0, 32)
    gf, mb = bench.ALGORITHMIC["s128"]
    assert abs(f["forward_hbm_frac"] - mb * 1e6 * 32 / 12.0e-3 / 8e12) < 1e-12
    assert abs(f["forward_fp32_frac_algorithmic"] - gf * 1e9 * 32 / 12.0e-3 / 157.3e12) < 1e-12
    assert abs(f["per_state"]["gflop"] - 35 * gf) < 1e-9 and abs(f["per_state"]["hbm_frac"] - 76.0 * 35 * mb * 1e6 / 8e12) < 1e-12
    assert bench.fractions("repaint128", 1.0, 1.0, 1) == {}
    prof = [{"name": "gn_bwd_kernel", "launches": 45, "total_ms": 5.5, "flops": 2e10, "bytes": 1.2e10},
            {"name": "conv_wino_kernel<WinoCfg<4>, false>", "launches": 53, "total_ms": 18.0, "flops": 4e12, "bytes": 1e10}]
    rows = bench.hbm_bound_rows(prof)
    assert [r["name"] for r in rows] == ["gn_bwd_kernel"] and abs(rows[0]["hbm_frac"] - round(1.2e10 / 5.5e-3 / 1e9, 1) / 8000.0) < 1e-3
    ro = bench.roofline_of(prof)
    assert ro["kernel"].startswith("conv_wino") and abs(ro["executed_over_algorithmic"] - 4 / 9) < 1e-12 and ro["frac"] < ro["direct_equivalent_frac"]


def test_plan_variants_are_per_plan_and_validated():
    """mcedm_unet_plan_set_variant (ABI 4): a field of the plan, validated on the host.  With the Winograd kernels switched off a
    decoder block's 1x1 skip projection is folded into conv1 again, so that plan's workspace layout differs from its sibling's --
    visible without a GPU."""
    cfg = orc.UNetConfig(ch=128, ch_mult=(1, 1, 1, 1), attn_resolutions=(16,))
    mk = lambda: L.Plan(cfg.in_channels, cfg.cond_channels, cfg.out_ch, cfg.ch, cfg.ch_mult, cfg.num_res_blocks,
                        cfg.attn_resolutions, cfg.resolution)
    pa, pb = mk(), mk()
    base = pb.workspace_bytes(2, 64, 64)
    assert pa.workspace_bytes(2, 64, 64) == base
    pa.set_variant("conv_wino", 0)
    assert pa.workspace_bytes(2, 64, 64) != base and pb.workspace_bytes(2, 64, 64) == base
    pa.set_variant("conv_wino", -1)
    assert pa.workspace_bytes(2, 64, 64) == base
    lib = L.load()
    assert lib.mcedm_unet_plan_set_variant(pa._h, 99, 1) != 0 and b"unknown switch" in lib.mcedm_last_error()
    assert lib.mcedm_unet_plan_set_variant(pa._h, 0, 7) != 0


def test_host_side_rejections_of_the_groupnorm_record_entries():
    """mcedm_op_conv_sums, mcedm_op_gn_coef_from_sums and mcedm_op_conv_gn refuse on the host, before any launch: null pointers, a
    record width other than 2 or 4, an output that is no whole number of records, and tables that cannot serve the GroupNorm asked
    for (the tiling does not cover the image, groups that are no whole records, records across the concat boundary) -- the last
    instead of the pass over the tensor that the plan's launcher falls back to."""
    lib = L._bind_ops()
    one = C.c_void_p(4096)
    til = lambda *t: (C.c_int * 5)(*t)      # noqa: E731
    out5 = til(0, 0, 0, 0, 0)

    def conv_sums(Cout=64, rc=4, gsum=one, tiling=out5, k=3, out=one, wpk=one):
        return lib.mcedm_op_conv_sums(one, None, 64, 0, None, 0, 0, 0, 16, 16, 16, 16, wpk, None, one, 0, None, 0, out, Cout, 2, k, gsum, rc,
                                      tiling, None)

    assert conv_sums(gsum=None) == -1 and _last() == "op_conv_sums: gsum / tiling_out is null"
    assert conv_sums(tiling=None) == -1 and _last() == "op_conv_sums: gsum / tiling_out is null"
    for rc in (3, 1, 8, -2):
        assert conv_sums(rc=rc) == -1 and _last() == f"op_conv_sums: gsum_rc = {rc}, records hold 4 (0 / 4) or 2 channels", rc
    assert conv_sums(Cout=66) == -1 and _last() == "op_conv_sums: Cout = 66 is not a whole number of 4-channel records"
    assert conv_sums(Cout=66, rc=0) == -1 and "4-channel records" in _last()
    assert conv_sums(Cout=65, rc=2) == -1 and _last() == "op_conv_sums: Cout = 65 is not a whole number of 2-channel records"
    assert conv_sums(k=2) == -1 and _last() == "op_conv_sums: k must be 1 or 3"
    assert conv_sums(out=None) == -1 and conv_sums(wpk=None) == -1 and _last() == "conv: null output / weights"
    assert list(out5) == [0] * 5                         # nothing was written

    t16 = til(4, 2, 8, 8, 4)                             # 16 x 16 in 8 x 8 tiles, quad records

    def coef(suma=one, sumb=None, ta=t16, tb=None, Ca=64, Cb=0, H=16, W=16, groups=16, gamma=one, beta=one, coef_out=one, B=2):
        return lib.mcedm_op_gn_coef_from_sums(suma, sumb, ta, tb, Ca, Cb, B, H, W, groups, gamma, beta, None, 0, 0, 1e-5, coef_out, None, None)

    def conv_gn(suma=one, sumb=None, ta=t16, tb=None, Ca=64, Cb=0, H=16, W=16, groups=16, gamma=one, beta=one, B=2, k=3):
        return lib.mcedm_op_conv_gn(one, one if Cb else None, Ca, Cb, suma, sumb, ta, tb, groups, gamma, beta, None, 0, 0, 1e-5, 1, 0, H, W,
                                    H, W, one, None, one, None, 0, one, 64, B, k, None)

    assert coef(coef_out=None) == -1 and _last() == "op_gn_coef_from_sums: null pointer"
    for who, call in (("op_gn_coef_from_sums", coef), ("op_conv_gn", conv_gn)):
        for kw in (dict(suma=None), dict(ta=None), dict(gamma=None), dict(beta=None)):
            assert call(**kw) == -1 and _last() == f"{who}: null pointer", (who, kw)
        assert call(B=0) == -1 and _last() == f"{who}: bad shape", who
        assert call(Cb=64, groups=32) == -1 and _last() == f"{who}: Cb = 64 without the second table", who
        assert call(Cb=64, groups=32, sumb=one) == -1 and "without the second table" in _last(), who
        assert call(groups=24) == -1 and _last() == f"{who}: C=64 not divisible by groups=24", who
        # tilings that do not cover the image: too few tiles, the wrong row length, a degenerate tile
        for bad in (til(3, 2, 8, 8, 4), til(4, 1, 8, 8, 4), til(4, 2, 8, 0, 4), til(0, 0, 0, 0, 0)):
            assert call(ta=bad) == -1 and "does not cover a 16 x 16 image" in _last(), (who, list(bad))
        assert call(H=20) == -1 and "does not cover a 20 x 16 image" in _last(), who
        # unusable records: rc = 3, 2-channel groups on quad records, a quad across the concat boundary, pairs | quads with 2-channel groups
        assert call(ta=til(4, 2, 8, 8, 3)) == -1 and _last() == f"{who}: records of 64 | 0 channels (3 / 3 per record) do not tile 16 groups", who
        assert call(groups=32) == -1 and _last() == f"{who}: records of 64 | 0 channels (4 / 4 per record) do not tile 32 groups", who
        assert call(Ca=66, Cb=62, sumb=one, tb=t16, groups=32) == -1 and "records of 66 | 62 channels (4 / 4 per record) do not tile 32" in _last(), who
        assert call(Cb=64, sumb=one, ta=til(4, 2, 8, 8, 2), tb=t16, groups=64) == -1 and "(2 / 4 per record) do not tile 64 groups" in _last(), who
    assert conv_gn(k=5) == -1 and _last() == "op_conv_gn: k must be 1 or 3"


def test_forced_8_wave_tile_refuses_pair_records():
    """The 8-wave kernel writes 4-channel records only.  The size heuristic never gives it a launch that asks for pairs; the forced tile
    (128, 16, 32) used to, and reported rc = 4 for a table the caller had sized, and would read, as pairs."""
    lib = L._bind_ops()
    one = C.c_void_p(4096)
    tiling = (C.c_int * 5)()
    L.set_conv_tile(128, 16, 32)
    try:
        rc = lib.mcedm_op_conv_sums(one, None, 128, 0, None, 0, 0, 0, 32, 32, 32, 32, one, None, one, 0, None, 0, one, 128, 2, 3, one, 2, tiling,
                                    None)
        msg = _last()
    finally:
        L.set_conv_tile()
    assert rc == -1 and "8-wave kernel" in msg and "4-channel statistics records only" in msg, (rc, msg)
    assert list(tiling) == [0] * 5
