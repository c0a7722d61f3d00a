"""ctypes binding of libmcedm_hip.so (include/mcedm_hip.h).

The product path has NO fallback: if the shared library is missing or a call fails, a
RuntimeError is raised.  Build it with ``python m-cedm_amd/build.py`` (hipcc, gfx950).
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, List, Optional, Sequence

import torch

from . import abi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MCEDM_LIB") or os.path.join(_HERE, "libmcedm_hip.so")   # MCEDM_LIB: A/B builds
# Every symbol, struct and constant of include/mcedm_hip.h, as abi.py reads them from the header itself: a new entry point is a
# prototype there, its definition, and a Python method here.  OP_EXPORTS: the kernel-level and measurement entries.
OP_EXPORTS = [n for n in abi.PROTOS if n.startswith(("mcedm_op_", "mcedm_prof_"))]
EXPORTS = [n for n in abi.PROTOS if n not in OP_EXPORTS]
ABI_VERSION, MAX_LEVELS = abi.CONSTS["MCEDM_ABI_VERSION"], abi.CONSTS["MCEDM_MAX_LEVELS"]
DX_NONE, DX_CAT, DX_ENC = abi.CONSTS["MCEDM_DX_NONE"], abi.CONSTS["MCEDM_DX_CAT"], abi.CONSTS["MCEDM_DX_ENC"]
GN_SYNC_WORDS, REDUCE_SCRATCH_BYTES = abi.CONSTS["MCEDM_GN_SYNC_WORDS"], abi.CONSTS["MCEDM_REDUCE_SCRATCH_BYTES"]
SWE_UNROLL_MAX_X = abi.CONSTS["MCEDM_SWE_UNROLL_MAX_X"]
# kernel families that exist in two forms (MCEDM_VARIANT_*), in index order
VARIANTS = {k[len("MCEDM_VARIANT_"):].lower(): v for k, v in sorted(abi.CONSTS.items(), key=lambda kv: kv[1])
            if k.startswith("MCEDM_VARIANT_")}
# The header's argument structs under the binding's names.  The host arrays behind a pointer field must outlive every call that
# reads the struct; who keeps them alive is noted with each.
UNetDesc = abi.STRUCTS["mcedm_unet_desc"]
SamplerDesc = abi.STRUCTS["mcedm_sampler_desc"]
GuidanceDesc = abi.STRUCTS["mcedm_guidance_desc"]
DdpmDesc = abi.STRUCTS["mcedm_ddpm_desc"]
DdpmCondDesc = abi.STRUCTS["mcedm_ddpm_cond_desc"]
RepaintDesc = abi.STRUCTS["mcedm_repaint_desc"]            # the caller, with the tensors repaint_desc returns next to the struct
DdimDesc = abi.STRUCTS["mcedm_ddim_desc"]                  # the caller, likewise (ddim_desc)
VpSamplerDesc = abi.STRUCTS["mcedm_vp_sampler_desc"]       # the Python object that built the struct (vp_sampler_desc)
CondDdimDesc = abi.STRUCTS["mcedm_cond_ddim_desc"]         # the Python object that built the struct (cond_ddim_desc)
# The sampler entries _PlanBase._sample_call drives, with the number of materialised-noise pointers each takes; every one
# has a "_rng" twin that takes ONE seed pointer in their place.  A new sampler is a row here and a method that names it.
SAMPLER_STEMS = {
    "mcedm_heun_sample": 1, "mcedm_heun_sample_guided": 1, "mcedm_heun_sample_dxcond": 1,
    "mcedm_vp_heun_sample": 1, "mcedm_ddpm_vp_heun_sample": 1, "mcedm_cond_ddim_sample": 1, "mcedm_ddpm_cond_ddim_sample": 1,
    "mcedm_ddim_repaint_sample": 1, "mcedm_repaint_sample": 2, "mcedm_ddpm_edm_heun_sample": 1,
}
# The PDE-guided (guide_dx) entries of the single-task samplers take the materialised draws AND the seed pointer in one signature
# (at most one of them non-NULL) behind a mcedm_guidance_desc*, and have no "_rng" twin: unguided stem -> guided entry.
GUIDED_ENTRIES = {
    "mcedm_vp_heun_sample": "mcedm_vp_heun_sample_guided", "mcedm_ddpm_vp_heun_sample": "mcedm_ddpm_vp_heun_sample_guided",
    "mcedm_cond_ddim_sample": "mcedm_cond_ddim_sample_guided", "mcedm_ddpm_cond_ddim_sample": "mcedm_ddpm_cond_ddim_sample_guided",
}
# The dx_cond entries of PlCondDdim's samplers on the ADM U-Net: the guided signature with the description of the dx residual
# (the network's dx input at the current state) in front of the guidance description, which may be NULL; no "_rng" twin either.
DXCOND_ENTRIES = {"mcedm_vp_heun_sample": "mcedm_vp_heun_sample_dxcond", "mcedm_cond_ddim_sample": "mcedm_cond_ddim_sample_dxcond"}

_lib = None


def load() -> C.CDLL:
    """Load the shared library (once).  Raises RuntimeError when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} not found: build it with `python m-cedm_amd/build.py` "
                           "(hipcc --offload-arch=gfx950); there is no CPU/PyTorch fallback")
    lib = C.CDLL(LIB_PATH)
    if lib.mcedm_version() != ABI_VERSION:           # the signatures and struct layouts applied below are those of this version
        raise RuntimeError(f"{LIB_PATH} implements ABI {lib.mcedm_version()}, this binding ABI {ABI_VERSION}: rebuild it with "
                           "`python m-cedm_amd/build.py`")
    for name, (restype, argtypes) in abi.PROTOS.items():
        fn = getattr(lib, name)          # AttributeError here == header/library drift
        fn.restype, fn.argtypes = restype, argtypes
    _lib = lib
    return lib


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        msg = load().mcedm_last_error().decode(errors="replace")
        raise RuntimeError(f"libmcedm_hip {what} failed ({rc}): {msg}")


def _ptr(t: Optional[torch.Tensor], dtype=torch.float32) -> Optional[int]:
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("libmcedm_hip needs device tensors (got a CPU tensor); there is no CPU fallback")
    if t.dtype != dtype:
        raise RuntimeError(f"expected dtype {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise RuntimeError("expected a contiguous tensor")
    return t.data_ptr()


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def sampler_desc(sp, sigma_data=1.0, net_sigma_min=0.002, net_sigma_max=80.0) -> SamplerDesc:
    """Build the C sampler description from the reference's ``sparams`` (attribute access, DictConfig or DotDict)."""
    return SamplerDesc(int(sp.timesteps), float(sp.sigma_min), float(sp.sigma_max), float(sp.rho), float(sp.S_churn),
                       float(sp.S_min), float(sp.S_max), float(sp.S_noise), float(sp.w), float(sigma_data),
                       float(net_sigma_min), float(net_sigma_max))


def desc_key(desc: C.Structure, skip: Sequence[str] = ()) -> tuple:
    """The hashable tuple of a ctypes description's fields, minus the pointer fields named in ``skip`` (their tables enter a
    cache key by value, where they can change): what tells two captured sampler calls apart."""
    return tuple(getattr(desc, f) for f, _ in desc._fields_ if f not in skip)


def edm_t_steps(sd: SamplerDesc) -> List[float]:
    arr = (C.c_double * (sd.timesteps + 1))()
    check(load().mcedm_edm_t_steps(C.byref(sd), arr), "edm_t_steps")
    return list(arr)


class Workspace:
    """Grow-only byte buffer on one device (the library never allocates device memory itself)."""

    def __init__(self):
        self.buf: Optional[torch.Tensor] = None

    def get(self, nbytes: int, device) -> torch.Tensor:
        if self.buf is None or self.buf.numel() < nbytes or self.buf.device != torch.device(device):
            self.buf = None
            self.buf = torch.empty(int(nbytes), dtype=torch.uint8, device=device)
        return self.buf


def _bucket_args(bucket_first, bucket_events, who: str):
    """(nb, firsts, evs) of a bucketed backward call; (0, None, None) without buckets."""
    if bucket_first is None:
        return 0, None, None
    nb = len(bucket_first)
    firsts = (C.c_int32 * nb)(*[int(f) for f in bucket_first])
    handles = [int(e.cuda_event) for e in bucket_events]
    if len(handles) != nb or not all(handles):
        raise RuntimeError(f"{who}: one created (recorded at least once) torch.cuda.Event per bucket is needed")
    return nb, firsts, (C.c_void_p * nb)(*handles)


def _seed_ptr(rng_seed: torch.Tensor, device, who: str) -> int:
    if rng_seed.dtype != torch.int64 or rng_seed.numel() != 1 or rng_seed.device != device:
        raise RuntimeError(f"{who}: rng_seed must be a one-element int64 tensor on the sampler's device")
    return rng_seed.data_ptr()


class _PlanBase:
    """What the two plan handles share.  _SYM: the prefix of the plan's own symbols (mcedm_unet / mcedm_ddpm); _WHAT: the
    prefix its entries carry in error messages ("" / "ddpm_")."""
    _SYM = _WHAT = ""

    def _adopt(self, lib, h) -> None:
        """Take ownership of the created plan handle and read its parameter table and packed size."""
        self._h, self._lib = h, lib
        self.param_names: List[str] = []
        self.param_shapes: List[tuple] = []
        for i in range(getattr(lib, self._SYM + "_param_count")(h)):
            name, numel, ndim, shape = C.c_char_p(), C.c_int64(), C.c_int32(), (C.c_int64 * 4)()
            check(getattr(lib, self._SYM + "_param_info")(h, i, C.byref(name), C.byref(numel), C.byref(ndim), C.byref(shape)))
            self.param_names.append(name.value.decode())
            self.param_shapes.append(tuple(shape[j] for j in range(ndim.value)))
        self.packed_bytes = self._bytes(self._SYM + "_packed_bytes", "")

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            getattr(self._lib, self._SYM + "_plan_destroy")(h)

    def set_variant(self, which: str, value: int = -1) -> None:
        """This plan's own choice for one kernel family (``VARIANTS``): 1 / 0, -1 = the process default (mcedm_op_set_* or the
        environment).  In force whenever one of THIS plan's entry points runs; other plans are not affected.  'conv_wino'
        also shapes the workspace layout: set it before the plan's first use."""
        fn = getattr(self._lib, self._SYM + "_plan_set_variant")
        check(fn(self._h, VARIANTS[which], int(value)), self._WHAT + "plan_set_variant")

    def _collect(self, params: Dict[str, torch.Tensor]) -> List[torch.Tensor]:
        """The plan's parameters out of ``params``, in table order, shapes checked."""
        tens = []
        for name, shape in zip(self.param_names, self.param_shapes):
            t = params[name]
            if tuple(t.shape) != shape:
                raise RuntimeError(f"parameter {name}: shape {tuple(t.shape)} != {shape}")
            tens.append(t.detach())
        return tens

    def _bytes(self, symbol: str, what: str, *args) -> int:
        """A size query ``symbol(plan, *args, &bytes)``; ``what`` names it in the error message."""
        sz = C.c_size_t()
        check(getattr(self._lib, symbol)(self._h, *args, C.byref(sz)), what)
        return sz.value

    # ---- the samplers ----------------------------------------------------------------------
    def _sample_call(self, who: str, stem: str, packed, head: Sequence, noise: Sequence[tuple], rng_seed, out, shapes: List[tuple],
                     dtype, return_last: bool, ws: Optional["Workspace"], nbytes: int, dims: tuple, device,
                     guidance: Optional["GuidanceDesc"] = None, dx_input: Optional["GuidanceDesc"] = None):
        """The call every sampler method makes: ``stem(plan, packed, *head, <draws>, <outputs>, return_last, workspace, bytes,
        *dims, stream)``.  noise: (name, tensor or None, dtype, shape) of each materialised draw ``stem`` takes; with rng_seed
        (device-side draws) ``stem + "_rng"`` runs instead, the one seed pointer in their place.  shapes: of the one or two
        ``dtype`` outputs, allocated here or checked against the caller's ``out`` (a graphed call's static tensors); returns
        the tensor, or the pair.  guidance: ``GUIDED_ENTRIES[stem]`` runs instead, the description behind the first entry of
        ``head`` (the sampler's) and the draws AND the seed pointer in its one signature.  dx_input (dx_cond plans, with or
        without guidance): ``DXCOND_ENTRIES[stem]`` runs, both descriptions behind the sampler's (guidance NULL when absent).  Every
        check runs before anything is enqueued."""
        if dx_input is not None and stem not in DXCOND_ENTRIES:
            raise RuntimeError(f"{who}: dx_input (dx_cond) is not built for {stem}")
        buf = (ws or Workspace()).get(nbytes, device)
        single = len(shapes) == 1
        if out is None:
            outs = [torch.empty(sh, dtype=dtype, device=device) for sh in shapes]
        else:
            outs = [out] if single else list(out)
            got = [tuple(o.shape) for o in outs]
            if got != shapes:
                raise RuntimeError(f"{who}: out has shape {got[0]}, expected {shapes[0]}" if single else
                                   f"{who}: out has shapes {got}, expected {shapes}")
        assert len(noise) == SAMPLER_STEMS[stem], stem
        for name, t, dt, shape in noise:
            if t is not None and (t.dtype != dt or tuple(t.shape) != tuple(shape)):
                raise RuntimeError(f"{who}: {name} must be {dt} {tuple(shape)}, got {t.dtype} {tuple(t.shape)}")
        if rng_seed is not None:
            if any(t is not None for _, t, _, _ in noise):
                raise RuntimeError(f"{who}: give {' / '.join(n[0] for n in noise)} (materialised draws) or rng_seed (device-side "
                                   "draws), not both")
            stem, draws = stem + "_rng", [_seed_ptr(rng_seed, device, who)]
        else:
            draws = [_ptr(t, dt) for _, t, dt, _ in noise]
        if guidance is not None or dx_input is not None:
            base = stem[:-len("_rng")] if rng_seed is not None else stem
            descs = (C.byref(guidance),) if dx_input is None else (C.byref(dx_input), None if guidance is None else C.byref(guidance))
            stem, head = (GUIDED_ENTRIES if dx_input is None else DXCOND_ENTRIES)[base], (head[0],) + descs + tuple(head[1:])
            draws = [_ptr(t, dt) for _, t, dt, _ in noise] + [_seed_ptr(rng_seed, device, who) if rng_seed is not None else None]
        check(getattr(self._lib, stem)(self._h, packed.data_ptr(), *head, *draws, *[_ptr(o, dtype) for o in outs], int(return_last),
                                       buf.data_ptr(), buf.numel(), *dims, _stream()), stem[len("mcedm_"):])
        return outs[0] if single else (outs[0], outs[1])

    # The two samplers of the single-task model run on either network: each plan supplies its symbol prefix (_WHAT), its size
    # queries, the trailing size arguments of its entries (_dims) and its input checks with the state's (H, W) (_state_hw).
    def vp_sample(self, packed, vd: "VpSamplerDesc", cond, init_noise, step_noise=None, return_last: bool = True,
                  ws: Optional["Workspace"] = None, rng_seed: Optional[torch.Tensor] = None,
                  out: Optional[torch.Tensor] = None, guidance: Optional["GuidanceDesc"] = None,
                  dx_input: Optional["GuidanceDesc"] = None) -> torch.Tensor:
        """mcedm_[ddpm_]vp_heun_sample (rng_seed None) / its _rng form; returns [B, 1 or N+1, H, W, in] float64 (``out``, when
        given: a graphed call's static tensor).  guidance: the PDE residual whose gradient at the denoised state corrects the
        slope (guide_dx): mcedm_[ddpm_]vp_heun_sample_guided, with the guided workspace.  dx_input (dx_cond plans of the ADM
        U-Net): the residual whose gradient at the current state, scaled by c_in, is the network's dx input:
        mcedm_vp_heun_sample_dxcond."""
        H, W = self._state_hw(init_noise, cond, "vp_sample")
        B, N = init_noise.shape[0], vd.timesteps
        return self._sample_call("vp_sample", f"mcedm_{self._WHAT}vp_heun_sample", packed,
                                 (C.byref(vd), _ptr(cond), _ptr(init_noise)),
                                 [("step_noise", step_noise, torch.float64, (N,) + tuple(init_noise.shape))], rng_seed, out,
                                 [(B, 1 if return_last else N + 1, H, W, self.in_channels)], torch.float64, return_last, ws,
                                 self.vp_sampler_workspace_bytes(B, H, W, guided=guidance is not None, **self._dx_kw(dx_input)),
                                 self._dims(B, H, W), init_noise.device, guidance=guidance, dx_input=dx_input)

    def cond_ddim_sample(self, packed, dd: "CondDdimDesc", cond, init_noise, eta_noise=None, return_last: bool = True,
                         ws: Optional["Workspace"] = None, out=None, rng_seed: Optional[torch.Tensor] = None,
                         guidance: Optional["GuidanceDesc"] = None, dx_input: Optional["GuidanceDesc"] = None):
        """mcedm_[ddpm_]cond_ddim_sample (PlCondDdim.sample on the device) -> (xs, x0_preds), both fp32 'b t h w c': S + 1 and S
        slots, or one each with return_last.  out: the pair to write into (a graphed call's static tensors).  rng_seed (int64 [1]
        on the device): the uniform draws of the eta != 0 steps are generated inside the step kernel (the _rng form, step k =
        draw k of uniform_fill) instead of being read from eta_noise [S, B, C, H, W].  guidance: the PDE residual whose gradient at
        each step's noisy state corrects et (guide_dx): mcedm_[ddpm_]cond_ddim_sample_guided, with the guided workspace.  dx_input
        (dx_cond plans of the ADM U-Net): the residual whose gradient at each step's noisy state is the network's dx input:
        mcedm_cond_ddim_sample_dxcond."""
        H, W = self._state_hw(init_noise, cond, "cond_ddim_sample")
        B, Cc = init_noise.shape[0], self.in_channels
        S = len(ddim_timesteps(dd.num_diffusion_timesteps, dd.timesteps, dd.skip_type))
        return self._sample_call("cond_ddim_sample", f"mcedm_{self._WHAT}cond_ddim_sample", packed,
                                 (C.byref(dd), _ptr(cond), _ptr(init_noise)),
                                 [("eta_noise", eta_noise, torch.float32, (S,) + tuple(init_noise.shape))], rng_seed, out,
                                 [(B, 1 if return_last else S + 1, H, W, Cc), (B, 1 if return_last else S, H, W, Cc)],
                                 torch.float32, return_last, ws,
                                 self.cond_ddim_workspace_bytes(B, H, W, guided=guidance is not None, **self._dx_kw(dx_input)),
                                 self._dims(B, H, W), init_noise.device, guidance=guidance, dx_input=dx_input)

    @staticmethod
    def _dx_kw(dx_input) -> dict:
        """The size queries' ``dxcond=True`` for a dx_cond call; nothing otherwise (the DDPM plan's queries have no such form)."""
        return {} if dx_input is None else {"dxcond": True}


class Plan(_PlanBase):
    """Host-side handle of one network architecture (mcedm_unet_plan_create)."""
    _SYM, _WHAT = "mcedm_unet", ""

    def __init__(self, in_channels: int, cond_channels: int, out_channels: int, ch: int, ch_mult: Sequence[int],
                 num_res_blocks: int, attn_resolutions: Sequence[int], resolution: int, channels_per_head: int = 64,
                 eps: float = 1e-5, dx_channels: int = 0, dx_mode: int = DX_NONE):
        lib = load()
        if len(ch_mult) > MAX_LEVELS or len(attn_resolutions) > MAX_LEVELS:
            raise RuntimeError("too many levels / attention resolutions")
        d = UNetDesc()
        d.in_channels, d.cond_channels, d.out_channels, d.ch = in_channels, cond_channels, out_channels, ch
        d.n_levels = len(ch_mult)
        for i, m in enumerate(ch_mult):
            d.ch_mult[i] = int(m)
        d.num_res_blocks, d.resolution = num_res_blocks, resolution
        d.n_attn_resolutions = len(attn_resolutions)
        for i, r in enumerate(attn_resolutions):
            d.attn_resolutions[i] = int(r)
        d.channels_per_head, d.eps = channels_per_head, eps
        d.dx_channels, d.dx_mode = int(dx_channels), int(dx_mode)
        self.dx_channels, self.dx_mode = int(dx_channels), int(dx_mode)
        self.desc = d
        h = C.c_void_p()
        check(lib.mcedm_unet_plan_create(C.byref(d), C.byref(h)), "plan_create")
        self._adopt(lib, h)
        self.in_channels, self.cond_channels, self.out_channels = in_channels, cond_channels, out_channels
        self.dropout, self._dropout_seed = 0.0, None           # what set_dropout last told the plan

    def set_dropout(self, p: float, rng_seed: Optional[torch.Tensor] = None) -> None:
        """Dropout of this plan's training entries (mcedm_unet_plan_set_dropout): 0 <= p < 1, p = 0 switches it off.  rng_seed: a
        one-element int64 DEVICE tensor the kernels read when the forward runs; the plan keeps a reference to it.  training=False
        calls and every sampler ignore the setting.  ``self.dropout`` / ``self._dropout_seed`` hold what the plan was last told."""
        p = float(p)
        if not (0.0 <= p < 1.0):                       # also NaN
            raise ValueError(f"dropout must lie in [0, 1), got {p}")
        if p > 0.0 and rng_seed is None:
            raise ValueError("dropout > 0 needs rng_seed, a one-element int64 tensor on the device")
        ptr = None
        if p > 0.0:
            if rng_seed.dtype != torch.int64 or rng_seed.numel() != 1:
                raise RuntimeError("set_dropout: rng_seed must be a one-element int64 tensor on the device")
            ptr = _ptr(rng_seed, torch.int64)
        check(self._lib.mcedm_unet_plan_set_dropout(self._h, p, ptr), "plan_set_dropout")
        self.dropout, self._dropout_seed = p, (rng_seed if p > 0.0 else None)

    # ---- derived weights ---------------------------------------------------------------
    def pack(self, params: Dict[str, torch.Tensor], packed: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Pack the named fp32 device parameters (keys = DhariwalUNet.state_dict() names)."""
        tens = self._collect(params)
        dev = tens[0].device
        if packed is None:
            packed = torch.empty(self.packed_bytes, dtype=torch.uint8, device=dev)
        arr = (C.c_void_p * len(tens))(*[_ptr(t) for t in tens])
        check(self._lib.mcedm_unet_pack_weights(self._h, arr, packed.data_ptr(), _stream()), "pack_weights")
        return packed

    # ---- sizes -----------------------------------------------------------------------------
    def workspace_bytes(self, B: int, H: int, W: int, training: bool = False) -> int:
        return self._bytes("mcedm_unet_workspace_bytes", "workspace_bytes", B, H, W, int(training))

    def sampler_workspace_bytes(self, B: int, H: int, W: int) -> int:
        return self._bytes("mcedm_sampler_workspace_bytes", "sampler_workspace_bytes", B, H, W)

    # ---- compute ---------------------------------------------------------------------------
    def _check_dx(self, x, dx):
        if dx is None:
            return
        if self.dx_mode == DX_NONE:
            raise RuntimeError("dx given to a plan without dx_cond")
        if tuple(dx.shape) != (x.shape[0], self.dx_channels, x.shape[2], x.shape[3]) or dx.dtype != torch.float32:
            raise RuntimeError(f"dx must be fp32 [B, {self.dx_channels}, H, W], got {tuple(dx.shape)} {dx.dtype}")

    def forward(self, packed, x, noise_labels, cond=None, x_scale=None, ws: Optional[Workspace] = None,
                training: bool = False, dx=None) -> torch.Tensor:
        self._check_dx(x, dx)
        B, _, H, W = x.shape
        n_noise = noise_labels.numel()
        ws = ws or Workspace()
        need = self.workspace_bytes(B, H, W, training)
        buf = ws.get(need, x.device)
        out = torch.empty((B, self.out_channels, H, W), dtype=torch.float32, device=x.device)
        check(self._lib.mcedm_unet_forward_dx(self._h, packed.data_ptr(), _ptr(x), _ptr(dx), _ptr(cond), _ptr(x_scale),
                                              _ptr(noise_labels), n_noise, _ptr(out), buf.data_ptr(), buf.numel(), B, H, W,
                                              int(training), _stream()), "unet_forward")
        return out

    def denoise(self, packed, x, sigma, cond=None, ws: Optional[Workspace] = None, training: bool = False,
                sigma_data: float = 1.0, want_F: bool = False, dx=None):
        self._check_dx(x, dx)
        B, _, H, W = x.shape
        n_sigma = sigma.numel()
        ws = ws or Workspace()
        buf = ws.get(self.workspace_bytes(B, H, W, training), x.device)
        D = torch.empty((B, self.out_channels, H, W), dtype=torch.float32, device=x.device)
        F = torch.empty_like(D) if want_F else None
        check(self._lib.mcedm_edm_denoise_dx(self._h, packed.data_ptr(), _ptr(x), _ptr(dx), _ptr(sigma), n_sigma, _ptr(cond),
                                             _ptr(D), _ptr(F), buf.data_ptr(), buf.numel(), B, H, W, int(training),
                                             float(sigma_data), _stream()), "edm_denoise")
        return (D, F) if want_F else D

    def grad_buckets(self, max_buckets: int) -> List[int]:
        """First parameter index of each gradient bucket, in the order the backward completes them (last one is 0)."""
        arr = (C.c_int32 * max(1, max_buckets))()
        n = C.c_int()
        check(self._lib.mcedm_unet_grad_buckets(self._h, int(max_buckets), arr, C.byref(n)), "grad_buckets")
        return [arr[i] for i in range(n.value)]

    def denoise_backward(self, packed, params: Dict[str, torch.Tensor], x, sigma, cond, dD, grads: Sequence[torch.Tensor],
                         ws: Workspace, sigma_data: float = 1.0, bucket_first: Optional[Sequence[int]] = None,
                         bucket_events: Optional[Sequence[torch.cuda.Event]] = None, dx=None) -> None:
        """Backward of denoise(..., training=True) on the SAME workspace: grads[i] <- dLoss/dparam_i (overwritten).
        With bucket_first / bucket_events the library records event k once every parameter >= bucket_first[k] is done."""
        self._check_dx(x, dx)
        B, _, H, W = x.shape
        buf = ws.get(self.workspace_bytes(B, H, W, True), x.device)
        parr = (C.c_void_p * len(self.param_names))(*[_ptr(params[n].detach()) for n in self.param_names])
        garr = (C.c_void_p * len(self.param_names))(*[_ptr(g) for g in grads])
        if dx is None and bucket_first is None:
            check(self._lib.mcedm_edm_denoise_backward(self._h, packed.data_ptr(), parr, _ptr(x), _ptr(sigma), sigma.numel(),
                                                       _ptr(cond), _ptr(dD), garr, buf.data_ptr(), buf.numel(), B, H, W,
                                                       float(sigma_data), _stream()), "edm_denoise_backward")
            return
        nb, firsts, evs = _bucket_args(bucket_first, bucket_events, "denoise_backward")
        check(self._lib.mcedm_edm_denoise_backward_dx(self._h, packed.data_ptr(), parr, _ptr(x), _ptr(dx), _ptr(sigma),
                                                      sigma.numel(), _ptr(cond), _ptr(dD), garr, buf.data_ptr(),
                                                      buf.numel(), B, H, W, float(sigma_data), nb, firsts, evs,
                                                      _stream()), "edm_denoise_backward_dx")

    def unet_backward(self, packed, params: Dict[str, torch.Tensor], x, noise_labels, cond, dF, grads: Sequence[torch.Tensor],
                      ws: Workspace, bucket_first: Optional[Sequence[int]] = None,
                      bucket_events: Optional[Sequence[torch.cuda.Event]] = None, dx=None) -> None:
        """Backward of forward(..., training=True) (x_scale None) on the SAME workspace, from dF = dLoss/d out:
        grads[i] <- dLoss/dparam_i (overwritten); bucket events as in denoise_backward.  dx: that forward's (dx_cond plans, which
        go through mcedm_unet_backward_dx whether or not this batch had a dx)."""
        self._check_dx(x, dx)
        B, _, H, W = x.shape
        buf = ws.get(self.workspace_bytes(B, H, W, True), x.device)
        parr = (C.c_void_p * len(self.param_names))(*[_ptr(params[n].detach()) for n in self.param_names])
        garr = (C.c_void_p * len(self.param_names))(*[_ptr(g) for g in grads])
        nb, firsts, evs = _bucket_args(bucket_first, bucket_events, "unet_backward")
        if self.dx_mode != DX_NONE:
            check(self._lib.mcedm_unet_backward_dx(self._h, packed.data_ptr(), parr, _ptr(x), _ptr(dx), _ptr(cond), None,
                                                   _ptr(noise_labels), noise_labels.numel(), _ptr(dF), garr, buf.data_ptr(),
                                                   buf.numel(), B, H, W, nb, firsts, evs, _stream()), "unet_backward_dx")
            return
        check(self._lib.mcedm_unet_backward_bucketed(self._h, packed.data_ptr(), parr, _ptr(x), _ptr(cond), None,
                                                     _ptr(noise_labels), noise_labels.numel(), _ptr(dF), garr, buf.data_ptr(),
                                                     buf.numel(), B, H, W, nb, firsts, evs, _stream()), "unet_backward")

    def vp_sampler_workspace_bytes(self, B: int, H: int, W: int, guided: bool = False, dxcond: bool = False) -> int:
        """dxcond: the size of mcedm_vp_heun_sample_dxcond, with or without guidance on top."""
        what = "vp_dxcond_workspace_bytes" if dxcond else "vp_guided_workspace_bytes" if guided else "vp_sampler_workspace_bytes"
        return self._bytes("mcedm_" + what, what, B, H, W)

    def cond_ddim_workspace_bytes(self, B: int, H: int, W: int, guided: bool = False, dxcond: bool = False) -> int:
        what = ("cond_ddim_dxcond_workspace_bytes" if dxcond else
                "cond_ddim_guided_workspace_bytes" if guided else "cond_ddim_workspace_bytes")
        return self._bytes("mcedm_" + what, what, B, H, W)

    def _dims(self, B: int, H: int, W: int) -> tuple:
        return B, H, W

    def _state_hw(self, x, cond, who: str):
        return x.shape[2], x.shape[3]

    def sample(self, packed, sd: SamplerDesc, cond, mask, init_noise, step_noise=None, return_last: bool = True,
               ws: Optional[Workspace] = None, out: Optional[torch.Tensor] = None,
               guidance: Optional["GuidanceDesc"] = None, dx_input: Optional["GuidanceDesc"] = None,
               rng_seed: Optional[torch.Tensor] = None) -> torch.Tensor:
        """dx_input: the residual whose gradient at the current state is the network's dx input (dx_cond plans).
        rng_seed: a one-element int64 DEVICE tensor -- the churn noise of every step is then generated inside the kernel that
        applies it (mcedm_heun_sample_rng and its _guided / _dxcond forms) instead of being read from step_noise
        [N, B, C, H, W] float64."""
        B, _, H, W = init_noise.shape
        N = sd.timesteps
        if dx_input is not None:
            if mask is not None:
                raise RuntimeError("sample: dx_cond sampling is the unmasked single-task sampler")
            stem = "mcedm_heun_sample_dxcond"
            head = (C.byref(sd), C.byref(dx_input), C.byref(guidance) if guidance is not None else None, _ptr(cond), _ptr(init_noise))
        elif guidance is not None:
            stem, head = "mcedm_heun_sample_guided", (C.byref(sd), C.byref(guidance), _ptr(cond), _ptr(mask), _ptr(init_noise))
        else:
            stem, head = "mcedm_heun_sample", (C.byref(sd), _ptr(cond), _ptr(mask), _ptr(init_noise))
        return self._sample_call("sample", stem, packed, head,
                                 [("step_noise", step_noise, torch.float64, (N,) + tuple(init_noise.shape))], rng_seed, out,
                                 [(B, 1 if return_last else N + 1, H, W, self.in_channels)], torch.float64, return_last, ws,
                                 self.sampler_workspace_bytes(B, H, W), (B, H, W), init_noise.device)


def repaint_desc(sp, edm_steps: torch.Tensor, alphas_ext: torch.Tensor, h_ch: int, u_ch: int):
    """C description of PlDdim.sample_edm's parameters (configs/diff_sampler/edm_sampler_inv.yaml) + the schedule tables
    (host fp32 tensors: get_edm_steps(), cumprod(1 - cat(0, betas))).  Returns (desc, keepalive)."""
    es = edm_steps.detach().to("cpu", torch.float32).contiguous()
    ae = alphas_ext.detach().to("cpu", torch.float32).contiguous()
    if ae.numel() != es.numel() + 1:
        raise RuntimeError("alphas_ext must have one more entry than edm_steps")
    d = RepaintDesc(int(sp.timesteps), float(sp.sigma_min), float(sp.sigma_max), float(sp.rho), float(sp.S_churn),
                    float(sp.S_min), float(sp.S_max), float(sp.S_noise), float(sp.w), int(sp.n_repeat), int(sp.n_time_h),
                    int(sp.n_time_u), int(h_ch), int(u_ch), int(es.numel()),
                    C.cast(es.data_ptr(), C.POINTER(C.c_float)), C.cast(ae.data_ptr(), C.POINTER(C.c_float)))
    return d, (es, ae)


def ddim_desc(sp, alphas_ext: torch.Tensor, h_ch: int, u_ch: int, self_cond: bool):
    """C description of PlDdim.sample_with_repeat's parameters (configs/diff_sampler/ddim_sampler*.yaml).  Returns (desc, keepalive)."""
    ae = alphas_ext.detach().to("cpu", torch.float32).contiguous()
    skip = {"uniform": 0, "quad": 1}.get(str(sp.skip_type))
    if skip is None:
        raise NotImplementedError(f"skip_type {sp.skip_type}")             # models/ddim.py:829-830
    d = DdimDesc(int(sp.timesteps), skip, float(sp.eta), int(sp.n_repeat), int(sp.n_time_h), int(sp.n_time_u), int(h_ch), int(u_ch),
                 int(ae.numel() - 1), int(bool(self_cond)), C.cast(ae.data_ptr(), C.POINTER(C.c_float)))
    return d, ae


def cond_ddim_desc(sp, alphas_ext: torch.Tensor, cond_channels: int, self_cond: bool) -> CondDdimDesc:
    """C description of PlCondDdim.sample's parameters (configs/diff_sampler/default.yaml, ddim_sampler*.yaml: timesteps,
    skip_type, eta, w) with the schedule table cumprod(1 - cat(0, betas)) attached (it must outlive every call that reads it)."""
    ae = alphas_ext.detach().to("cpu", torch.float32).contiguous()
    skip = {"uniform": 0, "quad": 1}.get(str(sp.skip_type))
    if skip is None:
        raise NotImplementedError(f"skip_type {sp.skip_type}")             # models/ddim.py:1469-1470
    w = getattr(sp, "w", None)
    d = CondDdimDesc(int(sp.timesteps), skip, float(sp.eta), 0.0 if w is None else float(w), int(cond_channels),
                     int(bool(self_cond)), int(ae.numel() - 1), C.cast(ae.data_ptr(), C.POINTER(C.c_float)))
    d._keep = ae
    return d


def ddim_timesteps(num_diffusion_timesteps: int, timesteps: int, skip_type) -> List[int]:
    """The timestep sequence of PlDdim.sample_with_repeat (models/ddim.py:823-830) as the device sampler walks it."""
    skip = {"uniform": 0, "quad": 1, 0: 0, 1: 1}.get(skip_type)
    if skip is None:
        raise NotImplementedError(f"skip_type {skip_type}")
    cnt = C.c_int()
    check(load().mcedm_ddim_timesteps(num_diffusion_timesteps, timesteps, skip, None, 0, C.byref(cnt)), "ddim_timesteps")
    arr = (C.c_int * cnt.value)()
    check(load().mcedm_ddim_timesteps(num_diffusion_timesteps, timesteps, skip, arr, cnt.value, C.byref(cnt)), "ddim_timesteps")
    return list(arr)


def repaint_schedule(rd: RepaintDesc) -> List[float]:
    arr = (C.c_double * (rd.timesteps + 1))()
    check(load().mcedm_repaint_schedule(C.byref(rd), arr), "repaint_schedule")
    return list(arr)


class DdpmPlan(_PlanBase):
    """Host-side handle of one DDPM U-Net (models/ddim_blocks.py Model; mcedm_ddpm_plan_create)."""
    _SYM, _WHAT = "mcedm_ddpm", "ddpm_"

    def __init__(self, in_channels: int, out_channels: int, ch: int, ch_mult: Sequence[int], num_res_blocks: int,
                 attn_resolutions: Sequence[int], resolution: int, self_cond: bool = True, eps: float = 1e-6,
                 cond_channels: int = 0, cat_cond: bool = False):
        """cond_channels > 0 (with cat_cond False): the cond_enc / combine_enc head of the single-task model
        (mcedm_ddpm_plan_create_cond); the parameter table then lists cond_enc.* / combine_enc.* behind conv_in.*.
        cond_channels > 0 with cat_cond True (needs self_cond False): no head, conv_in reads cat(cond, x) and its weight is
        [ch, cond_channels + in_channels, 3, 3]; forward_cat / edm_denoise / edm_sample take the raw conditioning."""
        lib = load()
        if len(ch_mult) > MAX_LEVELS or len(attn_resolutions) > MAX_LEVELS:
            raise RuntimeError("too many levels / attention resolutions")
        d = DdpmDesc()
        d.in_channels, d.out_channels, d.ch, d.n_levels = in_channels, out_channels, ch, len(ch_mult)
        for i, m in enumerate(ch_mult):
            d.ch_mult[i] = int(m)
        d.num_res_blocks, d.resolution, d.n_attn_resolutions = num_res_blocks, resolution, len(attn_resolutions)
        for i, r in enumerate(attn_resolutions):
            d.attn_resolutions[i] = int(r)
        d.self_cond, d.eps = int(bool(self_cond)), eps
        self.desc = d
        h = C.c_void_p()
        if cond_channels or cat_cond:
            cd = DdpmCondDesc(int(cond_channels), int(bool(cat_cond)))
            check(lib.mcedm_ddpm_plan_create_cond(C.byref(d), C.byref(cd), C.byref(h)), "ddpm_plan_create_cond")
        else:
            check(lib.mcedm_ddpm_plan_create(C.byref(d), C.byref(h)), "ddpm_plan_create")
        self._adopt(lib, h)
        self.in_channels, self.out_channels, self.resolution, self.ch = in_channels, out_channels, resolution, ch
        self.cond_channels = int(cond_channels)
        self.cat_cond = bool(cat_cond) and self.cond_channels > 0

    def pack(self, params: Dict[str, torch.Tensor], temb_freqs: torch.Tensor, packed: Optional[torch.Tensor] = None):
        """params keyed like Model.state_dict(); temb_freqs [ch/2] device fp32, built by the caller exactly as
        get_timestep_embedding does (models/ddim_blocks.py:22-24)."""
        tens = self._collect(params)
        if temb_freqs.numel() != self.ch // 2:
            raise RuntimeError("temb_freqs must have ch / 2 entries")
        if packed is None:
            packed = torch.empty(self.packed_bytes, dtype=torch.uint8, device=tens[0].device)
        arr = (C.c_void_p * len(tens))(*[_ptr(t) for t in tens])
        check(self._lib.mcedm_ddpm_pack_weights(self._h, arr, _ptr(temb_freqs), packed.data_ptr(), _stream()), "ddpm_pack_weights")
        return packed

    def workspace_bytes(self, B: int) -> int:
        return self._bytes("mcedm_ddpm_workspace_bytes", "ddpm_workspace_bytes", B)

    def repaint_workspace_bytes(self, B: int) -> int:
        return self._bytes("mcedm_repaint_workspace_bytes", "repaint_workspace_bytes", B)

    def _check_x(self, x):
        if tuple(x.shape[1:]) != (self.in_channels, self.resolution, self.resolution):
            raise RuntimeError(f"input {tuple(x.shape)} != [B, {self.in_channels}, {self.resolution}, {self.resolution}] "
                               "(the network asserts input size == resolution, ddim_blocks.py:411)")

    def forward(self, packed, x, t: float, ws: Optional[Workspace] = None, x_self_cond: Optional[torch.Tensor] = None) -> torch.Tensor:
        self._check_x(x)
        B = x.shape[0]
        ws = ws or Workspace()
        buf = ws.get(self.workspace_bytes(B), x.device)
        out = torch.empty((B, self.out_channels, self.resolution, self.resolution), dtype=torch.float32, device=x.device)
        if x_self_cond is not None:
            if tuple(x_self_cond.shape) != tuple(x.shape):
                raise RuntimeError("x_self_cond must have the shape of x")
            check(self._lib.mcedm_ddpm_forward_sc(self._h, packed.data_ptr(), _ptr(x), _ptr(x_self_cond), float(t), _ptr(out),
                                                  buf.data_ptr(), buf.numel(), B, _stream()), "ddpm_forward_sc")
            return out
        check(self._lib.mcedm_ddpm_forward(self._h, packed.data_ptr(), _ptr(x), float(t), _ptr(out), buf.data_ptr(),
                                           buf.numel(), B, _stream()), "ddpm_forward")
        return out

    # ---- the single-task model: the cond_enc head and the two samplers of PlCondDdim --------------------------------------
    def _check_cond(self, cond, who: str):
        R = self.resolution
        if cond is not None and tuple(cond.shape[1:]) != (self.cond_channels, R, R):
            raise RuntimeError(f"{who}: cond {tuple(cond.shape)} != [B, {self.cond_channels}, {R}, {R}]")

    def cond_map(self, packed, cond, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """mcedm_ddpm_cond_map: M(cond) [B, ch, R, R], what conv_in adds for this conditioning (once per sampler call)."""
        self._check_cond(cond, "cond_map")
        B, R = cond.shape[0], self.resolution
        if out is None:
            out = torch.empty((B, self.ch, R, R), dtype=torch.float32, device=cond.device)
        check(self._lib.mcedm_ddpm_cond_map(self._h, packed.data_ptr(), _ptr(cond), _ptr(out), B, _stream()), "ddpm_cond_map")
        return out

    def forward_cond(self, packed, x, t: float, cond_map=None, x_self_cond=None, ws: Optional[Workspace] = None) -> torch.Tensor:
        """mcedm_ddpm_forward_cond: Model.forward(x, t, cond, x_self_cond) with cond given as its map (None: cond None)."""
        self._check_x(x)
        B, R = x.shape[0], self.resolution
        if x_self_cond is not None and tuple(x_self_cond.shape) != tuple(x.shape):
            raise RuntimeError("x_self_cond must have the shape of x")
        if cond_map is not None and tuple(cond_map.shape) != (B, self.ch, R, R):
            raise RuntimeError(f"forward_cond: cond_map {tuple(cond_map.shape)} != {(B, self.ch, R, R)}")
        ws = ws or Workspace()
        buf = ws.get(self.workspace_bytes(B), x.device)
        out = torch.empty((B, self.out_channels, R, R), dtype=torch.float32, device=x.device)
        check(self._lib.mcedm_ddpm_forward_cond(self._h, packed.data_ptr(), _ptr(x), _ptr(x_self_cond), _ptr(cond_map), float(t),
                                                _ptr(out), buf.data_ptr(), buf.numel(), B, _stream()), "ddpm_forward_cond")
        return out

    # the size queries keep Plan's signatures (H, W: ignored, the state has the plan's resolution): GraphedVpSampler /
    # GraphedCondDdim and the Lightning module drive either network through them and through vp_sample / cond_ddim_sample
    def vp_sampler_workspace_bytes(self, B: int, H: Optional[int] = None, W: Optional[int] = None, guided: bool = False) -> int:
        what = "ddpm_vp_guided_workspace_bytes" if guided else "ddpm_vp_sampler_workspace_bytes"
        return self._bytes("mcedm_" + what, what, B)

    def cond_ddim_workspace_bytes(self, B: int, H: Optional[int] = None, W: Optional[int] = None, guided: bool = False) -> int:
        what = "ddpm_cond_ddim_guided_workspace_bytes" if guided else "ddpm_cond_ddim_workspace_bytes"
        return self._bytes("mcedm_" + what, what, B)

    def _dims(self, B: int, H: Optional[int] = None, W: Optional[int] = None) -> tuple:
        return (B,)

    def _state_hw(self, x, cond, who: str):
        self._check_x(x)
        self._check_cond(cond, who)
        return self.resolution, self.resolution

    # ---- the single-task EDM model on a cat_cond plan (PlCondEdm on Model) ----------------------------------------------
    def forward_cat(self, packed, x, t: float, cond=None, ws: Optional[Workspace] = None) -> torch.Tensor:
        """mcedm_ddpm_forward_cat: Model.forward(x, t, cond) with the raw conditioning in front of the state (None: zeros)."""
        self._check_x(x)
        self._check_cond(cond, "forward_cat")
        B, R = x.shape[0], self.resolution
        buf = (ws or Workspace()).get(self.workspace_bytes(B), x.device)
        out = torch.empty((B, self.out_channels, R, R), dtype=torch.float32, device=x.device)
        check(self._lib.mcedm_ddpm_forward_cat(self._h, packed.data_ptr(), _ptr(x), _ptr(cond), float(t), _ptr(out), buf.data_ptr(),
                                               buf.numel(), B, _stream()), "ddpm_forward_cat")
        return out

    def edm_denoise(self, packed, x, sigma: float, c_noise: float, cond=None, w: float = 0.0, sigma_data: float = 1.0,
                    ws: Optional[Workspace] = None, want_F: bool = False):
        """mcedm_ddpm_edm_denoise: PlCondEdm.get_denoised at one noise level; c_noise is the caller's fp32 ln(sigma) / 4."""
        self._check_x(x)
        self._check_cond(cond, "edm_denoise")
        B = x.shape[0]
        buf = (ws or Workspace()).get(self.workspace_bytes(B), x.device)
        D = torch.empty((B, self.out_channels, self.resolution, self.resolution), dtype=torch.float32, device=x.device)
        F = torch.empty_like(D) if want_F else None
        check(self._lib.mcedm_ddpm_edm_denoise(self._h, packed.data_ptr(), _ptr(x), _ptr(cond), float(sigma), float(c_noise), float(w),
                                               float(sigma_data), _ptr(D), _ptr(F), buf.data_ptr(), buf.numel(), B, _stream()),
              "ddpm_edm_denoise")
        return (D, F) if want_F else D

    def edm_sampler_workspace_bytes(self, B: int) -> int:
        return self._bytes("mcedm_ddpm_edm_sampler_workspace_bytes", "ddpm_edm_sampler_workspace_bytes", B)

    # ---- one timestep (noise level) per sample: the noising pass of training, forward only -------------------------------
    @property
    def temb_row_count(self) -> int:
        """mcedm_ddpm_temb_row_count: rows of the timestep table per sample (the ResnetBlocks' output channels)."""
        n = C.c_int32()
        check(self._lib.mcedm_ddpm_temb_row_count(self._h, C.byref(n)), "ddpm_temb_row_count")
        return int(n.value)

    def workspace_bytes_t(self, B: int) -> int:
        return self._bytes("mcedm_ddpm_workspace_bytes_t", "ddpm_workspace_bytes_t", B)

    @staticmethod
    def _check_levels(v, B: int, who: str, name: str):
        if not torch.is_tensor(v) or v.dtype != torch.float32 or v.dim() != 1 or v.numel() != B:
            raise RuntimeError(f"{who}: {name} must be a device fp32 tensor of shape [{B}] (one per sample; it is read on the device)")

    def temb_rows(self, packed, t: torch.Tensor) -> torch.Tensor:
        """mcedm_ddpm_temb_rows: [B, temb_row_count], per sample what the ResnetBlocks' conv1 add at t[b] (conv1.bias included),
        ordered as the *.temb_proj.weight entries of the parameter table."""
        if not torch.is_tensor(t) or t.dim() != 1 or t.numel() == 0:
            raise RuntimeError("temb_rows: t must be a non-empty 1-D tensor")
        B = t.numel()
        self._check_levels(t, B, "temb_rows", "t")
        out = torch.empty((B, self.temb_row_count), dtype=torch.float32, device=t.device)
        check(self._lib.mcedm_ddpm_temb_rows(self._h, packed.data_ptr(), _ptr(t), B, _ptr(out), _stream()), "ddpm_temb_rows")
        return out

    def forward_t(self, packed, x, t: torch.Tensor, x_self_cond=None, cond_map=None, cond=None, ws: Optional[Workspace] = None,
                  out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """mcedm_ddpm_forward_t: Model.forward(x, t [B], cond, x_self_cond), one timestep per sample, t a device tensor.  cond_map
        (of cond_map()) goes with a plan that has the head, cond (raw) with a cat_cond plan; None: cond None."""
        self._check_x(x)
        B, R = x.shape[0], self.resolution
        self._check_levels(t, B, "forward_t", "t")
        if x_self_cond is not None and tuple(x_self_cond.shape) != tuple(x.shape):
            raise RuntimeError("x_self_cond must have the shape of x")
        if cond_map is not None and tuple(cond_map.shape) != (B, self.ch, R, R):
            raise RuntimeError(f"forward_t: cond_map {tuple(cond_map.shape)} != {(B, self.ch, R, R)}")
        if cond is not None and (not self.cat_cond or cond.shape[0] != B):
            raise RuntimeError("forward_t: the raw conditioning [B, cond_channels, R, R] goes with a cat_cond plan (else pass cond_map)")
        self._check_cond(cond, "forward_t")
        buf = (ws or Workspace()).get(self.workspace_bytes_t(B), x.device)
        if out is None:
            out = torch.empty((B, self.out_channels, R, R), dtype=torch.float32, device=x.device)
        check(self._lib.mcedm_ddpm_forward_t(self._h, packed.data_ptr(), _ptr(x), _ptr(x_self_cond), _ptr(cond_map), _ptr(cond), _ptr(t),
                                             _ptr(out), buf.data_ptr(), buf.numel(), B, _stream()), "ddpm_forward_t")
        return out

    def edm_denoise_t(self, packed, x, sigma: torch.Tensor, cond=None, sigma_data: float = 1.0, ws: Optional[Workspace] = None,
                      want_F: bool = False):
        """mcedm_ddpm_edm_denoise_t: PlCondEdm.model_precond with one noise level per sample, sigma [B] a device tensor; every
        coefficient is computed on the device.  No guidance (edm_denoise serves it at one noise level)."""
        self._check_x(x)
        B = x.shape[0]
        self._check_levels(sigma, B, "edm_denoise_t", "sigma")
        if cond is not None and cond.shape[0] != B:
            raise RuntimeError("edm_denoise_t: cond must have the batch size of x")
        self._check_cond(cond, "edm_denoise_t")
        buf = (ws or Workspace()).get(self.workspace_bytes_t(B), x.device)
        D = torch.empty((B, self.out_channels, self.resolution, self.resolution), dtype=torch.float32, device=x.device)
        F = torch.empty_like(D) if want_F else None
        check(self._lib.mcedm_ddpm_edm_denoise_t(self._h, packed.data_ptr(), _ptr(x), _ptr(cond), _ptr(sigma), float(sigma_data), _ptr(D),
                                                 _ptr(F), buf.data_ptr(), buf.numel(), B, _stream()), "ddpm_edm_denoise_t")
        return (D, F) if want_F else D

    def edm_sample(self, packed, vd: "VpSamplerDesc", cond, init_noise, step_noise=None, return_last: bool = True,
                   ws: Optional[Workspace] = None, rng_seed: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
                   sigma_data: float = 1.0, guidance: Optional["GuidanceDesc"] = None) -> torch.Tensor:
        """mcedm_ddpm_edm_heun_sample (rng_seed None) / its _rng form: PlCondEdm.sample_edm on the device; returns
        [B, 1 or N+1, R, R, in] float64.  vd: vp_sampler_desc with t_hat as it is and c_noise = ln(sigma) / 4.  guidance: the PDE
        residual whose gradient at the denoised state corrects the slope (guide_dx)."""
        R = self._state_hw(init_noise, cond, "edm_sample")[0]
        B, N = init_noise.shape[0], vd.timesteps
        return self._sample_call("edm_sample", "mcedm_ddpm_edm_heun_sample", packed,
                                 (C.byref(vd), float(sigma_data), C.byref(guidance) if guidance is not None else None, _ptr(cond),
                                  _ptr(init_noise)),
                                 [("step_noise", step_noise, torch.float64, (N,) + tuple(init_noise.shape))], rng_seed, out,
                                 [(B, 1 if return_last else N + 1, R, R, self.in_channels)], torch.float64, return_last, ws,
                                 self.edm_sampler_workspace_bytes(B), (B,), init_noise.device)

    def ddim_workspace_bytes(self, B: int) -> int:
        return self._bytes("mcedm_ddim_workspace_bytes", "ddim_workspace_bytes", B)

    def ddim_repaint_sample(self, packed, dd: "DdimDesc", hu, init_noise, eta_noise=None, return_last: bool = True,
                            ws: Optional[Workspace] = None, rng_seed: Optional[torch.Tensor] = None, out=None):
        """PlDdim.sample_with_repeat on the device -> (xs, x0_preds), both fp32 'b t h w c'.  rng_seed (int64 [1] on the device):
        the uniform draws of the eta != 0 steps are generated inside the step kernel (mcedm_ddim_repaint_sample_rng, step k =
        draw k of uniform_fill) instead of being read from eta_noise.  out: the pair to write into (a graphed call's static
        tensors)."""
        self._check_x(hu)
        B, R, Cc = hu.shape[0], self.resolution, self.in_channels
        S = len(ddim_timesteps(dd.num_diffusion_timesteps, dd.timesteps, dd.skip_type))
        return self._sample_call("ddim_repaint_sample", "mcedm_ddim_repaint_sample", packed,
                                 (C.byref(dd), _ptr(hu), _ptr(init_noise)),
                                 [("eta_noise", eta_noise, torch.float32, (S,) + tuple(init_noise.shape))], rng_seed, out,
                                 [(B, 1 if return_last else S + 1, R, R, Cc), (B, 1 if return_last else S, R, R, Cc)],
                                 torch.float32, return_last, ws, self.ddim_workspace_bytes(B), (B,), hu.device)

    def denoise(self, packed, x, sigma: float, c_noise: float, ws: Optional[Workspace] = None, want_F: bool = False):
        self._check_x(x)
        B = x.shape[0]
        ws = ws or Workspace()
        buf = ws.get(self.workspace_bytes(B), x.device)
        D = torch.empty((B, self.out_channels, self.resolution, self.resolution), dtype=torch.float32, device=x.device)
        F = torch.empty_like(D) if want_F else None
        check(self._lib.mcedm_ddpm_denoise(self._h, packed.data_ptr(), _ptr(x), float(sigma), float(c_noise), _ptr(D), _ptr(F),
                                           buf.data_ptr(), buf.numel(), B, _stream()), "ddpm_denoise")
        return (D, F) if want_F else D

    def repaint_sample(self, packed, rd: RepaintDesc, hu, init_noise, step_noise=None, repeat_noise=None,
                       return_last: bool = True, ws: Optional[Workspace] = None, out: Optional[torch.Tensor] = None,
                       rng_seed: Optional[torch.Tensor] = None):
        """rng_seed (device int64 [1]): the per-step / per-loop noise is generated on the device from that seed
        (mcedm_repaint_sample_rng) instead of being read from step_noise / repeat_noise."""
        self._check_x(hu)
        B, R, N = hu.shape[0], self.resolution, rd.timesteps
        return self._sample_call("repaint_sample", "mcedm_repaint_sample", packed, (C.byref(rd), _ptr(hu), _ptr(init_noise)),
                                 [("step_noise", step_noise, torch.float64, (N,) + tuple(hu.shape)),
                                  ("repeat_noise", repeat_noise, torch.float64, (N, rd.n_repeat - 1) + tuple(hu.shape))],
                                 rng_seed, out, [(B, 1 if return_last else N + 1, R, R, self.in_channels)], torch.float64,
                                 return_last, ws, self.repaint_workspace_bytes(B), (B,), hu.device)


def normal_fill(out: torch.Tensor, rng_seed: torch.Tensor, draw: int) -> torch.Tensor:
    """out (fp64, contiguous) <- draw number `draw` of the device generator keyed by rng_seed (int64 [1] on the device)."""
    check(load().mcedm_normal_fill(_ptr(out, torch.float64), out.numel(), _ptr(rng_seed, torch.int64), int(draw), _stream()),
          "normal_fill")
    return out


def uniform_fill(out: torch.Tensor, rng_seed: torch.Tensor, draw: int) -> torch.Tensor:
    """out (fp32, contiguous) <- draw number `draw` of the device generator's UNIFORM stream keyed by rng_seed (int64 [1] on the
    device): multiples of 2^-24 in [0, 1), what the DDIM step kernels generate for themselves (mcedm_uniform_fill)."""
    check(load().mcedm_uniform_fill(_ptr(out), out.numel(), _ptr(rng_seed, torch.int64), int(draw), _stream()), "uniform_fill")
    return out


class _PinnedWorkspace:
    """Workspace view with a FIXED buffer: a captured graph bakes the pointer in, so the buffer must neither move nor be
    freed while the graph lives (the owner of the graph holds this object)."""

    def __init__(self, ws: Optional[Workspace], nbytes: int, device):
        self.buf = (ws or Workspace()).get(nbytes, device)

    def get(self, nbytes: int, device) -> torch.Tensor:
        if nbytes > self.buf.numel() or self.buf.device != torch.device(device):
            raise RuntimeError("graphed call: workspace request differs from the captured one")
        return self.buf


def _capture(run, dev) -> "torch.cuda.CUDAGraph":
    """Warm ``run`` up once off the capture (lazily initialised library state settles), then capture it into a HIP graph.
    capture_error_mode='thread_local': HIP calls of OTHER threads (DataLoader pin-memory thread, RCCL watchdog, logger
    hooks) during the long capture do not invalidate it."""
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        run()
    return graph


def _write_seed(dst: torch.Tensor, seed) -> None:
    """The key of a replay's device-side draws into the graph's int64 seed scalar: python int or int64 tensor."""
    if torch.is_tensor(seed):
        dst.copy_(seed.reshape(1))
    else:
        dst.fill_(int(seed))


def _copy_static(who: str, pairs) -> None:
    """Copy a replay's inputs into the graph's static buffers; (dst, src, name) with both None = not part of the capture."""
    for dst, src, name in pairs:
        if (dst is None) != (src is None):
            raise RuntimeError(f"{who}: '{name}' presence differs from the captured call")
        if dst is not None:
            dst.copy_(src)


class _GraphedCall:
    """What the Graphed* classes share: one sampler call captured ONCE into a HIP graph and replayed.  A subclass makes its
    static buffers (plain attributes), names the ones a replay copies into and defines ``_run``, the eager plan method on
    exactly those buffers; ``_capture_call`` pins the workspace and captures, ``_replay`` is every ``__call__``."""

    @staticmethod
    def _draws(dev, random: bool, device_noise: bool, shape: tuple, dtype):
        """(seed, noise) of a sampler that draws per step (``random``): the int64 device scalar that keys device-side draws
        (rewritten before each replay), or the static buffer materialised draws are copied into; (None, None) when it does not."""
        if not random:
            return None, None
        if device_noise:
            return torch.zeros(1, dtype=torch.int64, device=dev), None
        return None, torch.zeros(shape, dtype=dtype, device=dev)

    def _capture_call(self, dev, static: Dict[str, Optional[torch.Tensor]], ws: Optional[Workspace], nbytes: int) -> None:
        """static: the static input tensors under the names of ``__call__``'s arguments, in their order (None: not part of this
        capture).  ``self.seed`` and ``self.out`` are set by now."""
        self._static = static
        self.ws = _PinnedWorkspace(ws, nbytes, dev)
        self.graph = _capture(self._run, dev)

    def _replay(self, seed, *inputs):
        who = type(self).__name__
        if (self.seed is None) != (seed is None):
            raise RuntimeError(f"{who}: 'seed' goes with device_noise=True instances of a sampler that draws (and only with them)")
        if seed is not None:
            _write_seed(self.seed, seed)
        _copy_static(who, [(dst, src, name) for (name, dst), src in zip(self._static.items(), inputs)])
        self.graph.replay()
        return self.out


class GraphedSampler(_GraphedCall):
    """The whole Heun sampling call (every U-Net evaluation and state update of mcedm_heun_sample: ~4000 launches at
    18 steps) captured ONCE into a HIP graph and replayed.  The library never allocates or synchronises and the sigma
    schedule is host-side arithmetic baked into kernel arguments, so a replay is exact; inputs are copied into static
    buffers first.  Shapes, sampler parameters and the packed-weight buffer are fixed per instance (re-packing weights
    in place into the same buffer is fine).  ``ws``: the caller's workspace to borrow (replays and eager calls of one
    module are serial on one stream, so one buffer serves both); the instance keeps the buffer it captured with alive."""

    def __init__(self, plan: "Plan", packed: torch.Tensor, sd: SamplerDesc, B: int, H: int, W: int, masked: bool = True,
                 has_cond: bool = True, churn: bool = False, return_last: bool = True, ws: Optional[Workspace] = None,
                 guidance: Optional["GuidanceDesc"] = None, dx_input: Optional["GuidanceDesc"] = None, device_noise: bool = False):
        """churn with device_noise: the per-step draws are generated inside the sampler's kernels from ``self.seed`` (an int64
        device scalar the call rewrites before each replay) -- no [N, B, C, H, W] float64 buffer, fresh noise per replay."""
        dev = packed.device
        self.plan, self.packed, self.sd, self.return_last = plan, packed, sd, return_last
        self.guidance, self.dx_input = guidance, dx_input      # host-side descriptions, baked into the captured kernel arguments
        C = plan.in_channels
        self.cond = torch.zeros((B, plan.cond_channels, H, W), device=dev) if has_cond else None
        self.mask = torch.zeros((B, C, H, W), device=dev) if masked else None
        self.init = torch.zeros((B, C, H, W), device=dev)
        self.seed, self.step_noise = self._draws(dev, churn, device_noise, (sd.timesteps, B, C, H, W), torch.float64)
        self.out = torch.empty((B, 1 if return_last else sd.timesteps + 1, H, W, C), dtype=torch.float64, device=dev)
        self._capture_call(dev, {"cond": self.cond, "mask": self.mask, "init_noise": self.init, "step_noise": self.step_noise},
                           ws, plan.sampler_workspace_bytes(B, H, W))

    def _run(self):
        self.plan.sample(self.packed, self.sd, self.cond, self.mask, self.init, self.step_noise, self.return_last, self.ws,
                         out=self.out, guidance=self.guidance, dx_input=self.dx_input, rng_seed=self.seed)

    def __call__(self, cond, mask, init_noise, step_noise=None, seed=None) -> torch.Tensor:
        """Returns the instance's static output tensor (overwritten by the next call).  seed (device-noise instances): python
        int or int64 tensor, the key of this call's churn draws."""
        return self._replay(seed, cond, mask, init_noise, step_noise)


class GraphedRepaint(_GraphedCall):
    """mcedm_repaint_sample_rng captured once and replayed: the whole RePaint call (timesteps x n_repeat Heun updates:
    ~80 000 launches at BASELINE config 5) is one HIP graph.  The noise is generated on the device from the seed in
    ``self.seed``, which the host rewrites before each replay, so every replay draws fresh noise."""

    def __init__(self, plan: "DdpmPlan", packed: torch.Tensor, rd: RepaintDesc, keep, B: int, return_last: bool = True,
                 ws: Optional[Workspace] = None):
        dev = packed.device
        self.plan, self.packed, self.rd, self._keep, self.return_last = plan, packed, rd, keep, return_last
        S, Cc = plan.resolution, plan.in_channels
        self.hu = torch.zeros((B, Cc, S, S), device=dev)
        self.init = torch.zeros((B, Cc, S, S), device=dev)
        self.seed = torch.zeros(1, dtype=torch.int64, device=dev)
        self.out = torch.empty((B, 1 if return_last else rd.timesteps + 1, S, S, Cc), dtype=torch.float64, device=dev)
        self._capture_call(dev, {"hu": self.hu, "init_noise": self.init}, ws, plan.repaint_workspace_bytes(B))

    def _run(self):
        self.plan.repaint_sample(self.packed, self.rd, self.hu, self.init, None, None, self.return_last, self.ws, out=self.out,
                                 rng_seed=self.seed)

    def __call__(self, hu, init_noise, seed) -> torch.Tensor:
        """seed: python int or int64 tensor.  Returns the instance's static output tensor."""
        return self._replay(seed, hu, init_noise)


class GraphedCondDdim(_GraphedCall):
    """mcedm_cond_ddim_sample captured once and replayed, like GraphedSampler: the schedule is host arithmetic baked into the
    kernel arguments, the inputs (cond, init_noise and, with eta != 0, the uniform draws of every step) are copied into static
    buffers first.  device_noise (with eta != 0): mcedm_cond_ddim_sample_rng instead -- the step kernel generates the draws from
    ``self.seed`` (an int64 device scalar the call rewrites before each replay) and no [S, B, C, H, W] buffer exists.  Returns the
    instance's static (xs, x0_preds), overwritten by the next call."""

    def __init__(self, plan: "Plan", packed: torch.Tensor, dd: CondDdimDesc, B: int, H: int, W: int, stochastic: bool,
                 return_last: bool = True, ws: Optional[Workspace] = None, device_noise: bool = False,
                 guidance: Optional["GuidanceDesc"] = None, dx_input: Optional["GuidanceDesc"] = None):
        dev = packed.device
        self.plan, self.packed, self.dd, self.return_last = plan, packed, dd, return_last
        self.guidance, self.dx_input = guidance, dx_input      # host-side descriptions (guide_dx, dx_cond), baked into the captured kernel arguments
        Cc, S = plan.in_channels, len(ddim_timesteps(dd.num_diffusion_timesteps, dd.timesteps, dd.skip_type))
        self.cond = torch.zeros((B, dd.cond_channels, H, W), device=dev) if dd.cond_channels > 0 else None
        self.init = torch.zeros((B, Cc, H, W), device=dev)
        self.seed, self.eta_noise = self._draws(dev, stochastic, device_noise, (S, B, Cc, H, W), torch.float32)
        self.out = (torch.empty((B, 1 if return_last else S + 1, H, W, Cc), device=dev),
                    torch.empty((B, 1 if return_last else S, H, W, Cc), device=dev))
        self._capture_call(dev, {"cond": self.cond, "init_noise": self.init, "eta_noise": self.eta_noise}, ws,
                           plan.cond_ddim_workspace_bytes(B, H, W, guided=guidance is not None, **plan._dx_kw(dx_input)))

    def _run(self):
        self.plan.cond_ddim_sample(self.packed, self.dd, self.cond, self.init, self.eta_noise, self.return_last, self.ws, out=self.out,
                                   rng_seed=self.seed, guidance=self.guidance, dx_input=self.dx_input)

    def __call__(self, cond, init_noise, eta_noise=None, seed=None):
        return self._replay(seed, cond, init_noise, eta_noise)


class GraphedDdimRepaint(_GraphedCall):
    """mcedm_ddim_repaint_sample (device_noise False) or mcedm_ddim_repaint_sample_rng (True) captured once and replayed: every
    network pass and elementwise kernel of PlDdim.sample_with_repeat is one HIP graph.  With eta != 0 the uniform draws are either
    copied into a static [S, B, C, R, R] buffer or generated by the step kernel from ``self.seed``.  ``keep``: the host tables the
    description points at.  Returns the instance's static (xs, x0_preds), overwritten by the next call."""

    def __init__(self, plan: "DdpmPlan", packed: torch.Tensor, dd: DdimDesc, keep, B: int, stochastic: bool, return_last: bool = True,
                 ws: Optional[Workspace] = None, device_noise: bool = False):
        dev = packed.device
        self.plan, self.packed, self.dd, self._keep, self.return_last = plan, packed, dd, keep, return_last
        R, Cc = plan.resolution, plan.in_channels
        S = len(ddim_timesteps(dd.num_diffusion_timesteps, dd.timesteps, dd.skip_type))
        self.hu = torch.zeros((B, Cc, R, R), device=dev)
        self.init = torch.zeros((B, Cc, R, R), device=dev)
        self.seed, self.eta_noise = self._draws(dev, stochastic, device_noise, (S, B, Cc, R, R), torch.float32)
        self.out = (torch.empty((B, 1 if return_last else S + 1, R, R, Cc), device=dev),
                    torch.empty((B, 1 if return_last else S, R, R, Cc), device=dev))
        self._capture_call(dev, {"hu": self.hu, "init_noise": self.init, "eta_noise": self.eta_noise}, ws,
                           plan.ddim_workspace_bytes(B))

    def _run(self):
        self.plan.ddim_repaint_sample(self.packed, self.dd, self.hu, self.init, self.eta_noise, self.return_last, self.ws,
                                      rng_seed=self.seed, out=self.out)

    def __call__(self, hu, init_noise, eta_noise=None, seed=None):
        return self._replay(seed, hu, init_noise, eta_noise)


class GraphedVpSampler(_GraphedCall):
    """mcedm_vp_heun_sample (device_noise False) or mcedm_vp_heun_sample_rng (True) captured once and replayed: the ~2 N network
    evaluations and state updates of PlCondDdim.sample_edm are one HIP graph.  churn: some step of ``vd`` has t_hat > t_cur; its
    normal draws are either copied into a static [N, B, C, H, W] float64 buffer or generated by the churn kernel from
    ``self.seed``.  Returns the instance's static output tensor, overwritten by the next call."""

    def __init__(self, plan: "Plan", packed: torch.Tensor, vd: VpSamplerDesc, B: int, H: int, W: int, has_cond: bool, churn: bool,
                 return_last: bool = True, ws: Optional[Workspace] = None, device_noise: bool = False,
                 guidance: Optional["GuidanceDesc"] = None, dx_input: Optional["GuidanceDesc"] = None):
        dev = packed.device
        self.plan, self.packed, self.vd, self.return_last = plan, packed, vd, return_last
        self.guidance, self.dx_input = guidance, dx_input      # host-side descriptions (guide_dx, dx_cond), baked into the captured kernel arguments
        Cc = plan.in_channels
        self.cond = torch.zeros((B, vd.cond_channels, H, W), device=dev) if has_cond else None
        self.init = torch.zeros((B, Cc, H, W), device=dev)
        self.seed, self.step_noise = self._draws(dev, churn, device_noise, (vd.timesteps, B, Cc, H, W), torch.float64)
        self.out = torch.empty((B, 1 if return_last else vd.timesteps + 1, H, W, Cc), dtype=torch.float64, device=dev)
        self._capture_call(dev, {"cond": self.cond, "init_noise": self.init, "step_noise": self.step_noise}, ws,
                           plan.vp_sampler_workspace_bytes(B, H, W, guided=guidance is not None, **plan._dx_kw(dx_input)))

    def _run(self):
        self.plan.vp_sample(self.packed, self.vd, self.cond, self.init, self.step_noise, self.return_last, self.ws,
                            rng_seed=self.seed, out=self.out, guidance=self.guidance, dx_input=self.dx_input)

    def __call__(self, cond, init_noise, step_noise=None, seed=None) -> torch.Tensor:
        return self._replay(seed, cond, init_noise, step_noise)


class GraphedDdpmEdmSampler(_GraphedCall):
    """mcedm_ddpm_edm_heun_sample (device_noise False) or its _rng form (True) captured once and replayed: the ~2 N network
    evaluations (twice that with classifier-free guidance), the PDE-guidance gradients and the state updates of PlCondEdm.sample_edm
    on the DDPM U-Net are one HIP graph.  Returns the instance's static output tensor, overwritten by the next call."""

    def __init__(self, plan: "DdpmPlan", packed: torch.Tensor, vd: VpSamplerDesc, B: int, has_cond: bool, churn: bool,
                 return_last: bool = True, ws: Optional[Workspace] = None, device_noise: bool = False, sigma_data: float = 1.0,
                 guidance: Optional["GuidanceDesc"] = None):
        dev = packed.device
        self.plan, self.packed, self.vd, self.return_last = plan, packed, vd, return_last
        self.sigma_data, self.guidance = sigma_data, guidance      # host-side, baked into the captured kernel arguments
        R, Cc = plan.resolution, plan.in_channels
        self.cond = torch.zeros((B, plan.cond_channels, R, R), device=dev) if has_cond else None
        self.init = torch.zeros((B, Cc, R, R), device=dev)
        self.seed, self.step_noise = self._draws(dev, churn, device_noise, (vd.timesteps, B, Cc, R, R), torch.float64)
        self.out = torch.empty((B, 1 if return_last else vd.timesteps + 1, R, R, Cc), dtype=torch.float64, device=dev)
        self._capture_call(dev, {"cond": self.cond, "init_noise": self.init, "step_noise": self.step_noise}, ws,
                           plan.edm_sampler_workspace_bytes(B))

    def _run(self):
        self.plan.edm_sample(self.packed, self.vd, self.cond, self.init, self.step_noise, self.return_last, self.ws,
                             rng_seed=self.seed, out=self.out, sigma_data=self.sigma_data, guidance=self.guidance)

    def __call__(self, cond, init_noise, step_noise=None, seed=None) -> torch.Tensor:
        return self._replay(seed, cond, init_noise, step_noise)


def graphed_or_eager(cache: dict, key, build, eager, max_entries: int = 2):
    """Replay the cached graph for ``key`` (building it with ``build()`` on first use, at most ``max_entries`` kept, oldest
    evicted) and return ``fn`` such that fn(*args) runs the call; if the capture fails (another thread's HIP call under a
    global capture mode, an out-of-memory while the static buffers are made) the entry is dropped, the failure is
    remembered for this key and ``eager`` is returned instead: the evaluation loop goes on without a graph."""
    hit = cache.get(key)
    if hit is not None:
        return hit if hit != "eager" else eager
    while len(cache) >= max_entries:
        cache.pop(next(iter(cache)))
    try:
        cache[key] = build()
    except (RuntimeError, torch.cuda.OutOfMemoryError) as e:
        import warnings
        warnings.warn(f"HIP-graph capture of the sampling call failed ({str(e)[:200]}); running it eagerly")
        torch.cuda.synchronize()
        cache[key] = "eager"
        return eager
    return cache[key]


# ---- flat-buffer training helpers -------------------------------------------------------------
def edm_noise_inputs(x, mask, noise, rnd_normal, P_mean=-1.2, P_std=1.2):
    B, Cc, H, W = x.shape
    x_noise = torch.empty_like(x)
    sigma = torch.empty(B, dtype=torch.float32, device=x.device)
    check(load().mcedm_edm_noise_inputs(_ptr(x), _ptr(mask), _ptr(noise), _ptr(rnd_normal), B, Cc, H, W, P_mean, P_std,
                                        _ptr(x_noise), _ptr(sigma), _stream()), "edm_noise_inputs")
    return x_noise, sigma


def eps_noise_inputs(x, noise, t, sqrt_ab, sqrt_1mab):
    """x_noise = x sqrt(a_t) + noise sqrt(1 - a_t) and the labels t.float() (mcedm_eps_noise_inputs); t int64 on the device."""
    B, Cc, H, W = x.shape
    if t.dtype != torch.int64 or t.numel() != B or not t.is_contiguous():
        raise RuntimeError("eps_noise_inputs: t must be a contiguous int64 tensor of B timesteps")
    n = sqrt_ab.numel()
    if int(t.min()) < 0 or int(t.max()) >= n:
        raise RuntimeError(f"eps_noise_inputs: timesteps outside [0, {n})")
    x_noise = torch.empty_like(x)
    labels = torch.empty(B, dtype=torch.float32, device=x.device)
    check(load().mcedm_eps_noise_inputs(_ptr(x), _ptr(noise), _ptr(t, torch.int64), _ptr(sqrt_ab), _ptr(sqrt_1mab), n, B, Cc, H,
                                        W, _ptr(x_noise), _ptr(labels), _stream()), "eps_noise_inputs")
    return x_noise, labels


def eps_self_cond(out, cond, cond_channels, in_channels, x_noise=None, F0=None, t=None, sqrt_ab=None, sqrt_1mab=None):
    """out [B, cond_channels + in_channels, H, W] <- cat(cond or 0, x_sc or 0) (mcedm_eps_self_cond)."""
    B, _, H, W = out.shape
    n = 0 if sqrt_ab is None else sqrt_ab.numel()
    check(load().mcedm_eps_self_cond(_ptr(x_noise), _ptr(F0), _ptr(t, torch.int64), _ptr(sqrt_ab), _ptr(sqrt_1mab), n, _ptr(cond),
                                     cond_channels, in_channels, B, H, W, _ptr(out), _stream()), "eps_self_cond")
    return out


def eps_loss(F, eps, want_grad=True, scratch: Optional[torch.Tensor] = None):
    B, Cc, H, W = F.shape
    loss = torch.empty(1, dtype=torch.float32, device=F.device)
    dF = torch.empty_like(F) if want_grad else None
    scratch = reduce_scratch(F.device) if scratch is None else scratch
    check(load().mcedm_eps_loss(_ptr(F), _ptr(eps), B, Cc, H, W, _ptr(loss), _ptr(dF), scratch.data_ptr(),
                                scratch.numel() * scratch.element_size(), _stream()), "eps_loss")
    return loss, dF


def vp_sampler_desc(timesteps, cond_channels, t_steps, t_hat, c_noise, S_noise, w) -> VpSamplerDesc:
    """The struct with its host arrays attached (they must outlive every call that reads it)."""
    ts = (C.c_double * (timesteps + 1))(*[float(v) for v in t_steps])
    th = (C.c_double * timesteps)(*[float(v) for v in t_hat])
    cn = (C.c_float * (2 * timesteps))(*[float(v) for v in c_noise])
    d = VpSamplerDesc(int(timesteps), int(cond_channels), ts, th, cn, float(S_noise), float(w))
    d._keep = (ts, th, cn)
    return d


_RED_SCRATCH = {}


def reduce_scratch(device, stream=None) -> torch.Tensor:
    """MCEDM_REDUCE_SCRATCH_BYTES of device memory for the fixed-order sums of edm_loss / sqnorm, one area per (device, stream):
    the library owns no device state (ABI 3), and calls on different streams must not share an area."""
    if torch.cuda.is_current_stream_capturing():      # belongs to the graph being captured (its private pool), never cached
        return torch.empty(REDUCE_SCRATCH_BYTES, dtype=torch.uint8, device=device)
    key = (torch.device(device).index, int(_stream() or 0) if stream is None else int(stream))
    buf = _RED_SCRATCH.get(key)
    if buf is None:
        buf = _RED_SCRATCH[key] = torch.empty(REDUCE_SCRATCH_BYTES, dtype=torch.uint8, device=device)
    return buf


def edm_loss(D, x, mask, sigma, sigma_data=1.0, want_grad=True, scratch: Optional[torch.Tensor] = None):
    B, Cc, H, W = D.shape
    loss = torch.empty(1, dtype=torch.float32, device=D.device)
    dD = torch.empty_like(D) if want_grad else None
    scratch = reduce_scratch(D.device) if scratch is None else scratch
    check(load().mcedm_edm_loss(_ptr(D), _ptr(x), _ptr(mask), _ptr(sigma), B, Cc, H, W, float(sigma_data), _ptr(loss),
                                _ptr(dD), scratch.data_ptr(), scratch.numel() * scratch.element_size(), _stream()), "edm_loss")
    return loss, dD


def pde_train_loss(gd: GuidanceDesc, D, h, gt=None, w=None, dD=None, scratch: Optional[torch.Tensor] = None):
    """The PDE term of PlCondEdm.training_step (mcedm_pde_train_loss): ``(pde_loss, dD)`` with ``pde_loss`` one fp32 (not multiplied
    by ``gd.weight`` = pde_loss_lambda) and ``dD += gd.weight * d pde_loss / d D`` in place; ``dD=None``: the value alone.
    ``D`` [B, 1, H, W]; ``h`` the normalised conditioning field as (B, H, W) or (B, H, W, 1), any strides (read in place);
    ``gt`` None (the state itself) or un-normalised (B, H, W, 2); ``w`` [B] per-sample factors or None."""
    B, Cc, H, W = D.shape
    if Cc != 1:
        raise RuntimeError(f"pde_train_loss: D must be [B, 1, H, W], got {tuple(D.shape)}")
    hv = h[..., 0] if h.dim() == 4 else h
    if tuple(hv.shape) != (B, H, W) or h.dim() == 4 and h.shape[3] != 1:
        raise RuntimeError(f"pde_train_loss: h must be {(B, H, W)} or {(B, H, W, 1)}, got {tuple(h.shape)}")
    if not hv.is_cuda or hv.dtype != torch.float32:
        raise RuntimeError("pde_train_loss: h must be an fp32 device tensor")
    if gt is not None and tuple(gt.shape) != (B, H, W, 2):
        raise RuntimeError(f"pde_train_loss: gt must be {(B, H, W, 2)}, got {tuple(gt.shape)}")
    if w is not None and w.numel() != B:
        raise RuntimeError(f"pde_train_loss: w must hold {B} factors, got {w.numel()}")
    if dD is not None and tuple(dD.shape) != tuple(D.shape):
        raise RuntimeError(f"pde_train_loss: dD must be {tuple(D.shape)}, got {tuple(dD.shape)}")
    loss = torch.empty(1, dtype=torch.float32, device=D.device)
    scratch = reduce_scratch(D.device) if scratch is None else scratch
    lib = load()
    nbytes = lib.mcedm_pde_train_scratch_bytes(C.byref(gd), B, H, W) if dD is not None else 0
    pde_scratch = torch.empty(nbytes, dtype=torch.uint8, device=D.device) if nbytes else None
    check(lib.mcedm_pde_train_loss(C.byref(gd), _ptr(D), hv.data_ptr(), hv.stride(0), hv.stride(1), hv.stride(2), _ptr(gt),
                                   _ptr(w), B, H, W, _ptr(loss), _ptr(dD), None if pde_scratch is None else pde_scratch.data_ptr(),
                                   nbytes, scratch.data_ptr(), scratch.numel() * scratch.element_size(), _stream()),
          "pde_train_loss")
    return loss, dD


# ---- PDE residuals (models/pde_loss.py) -------------------------------------------------------
def swe_fv_step(s_t: torch.Tensor, half_dt: float, dx: float) -> torch.Tensor:
    """SweFvLoss.f_t_swp1d on (b, t, x, 2) fp32 states."""
    B, T, X, _ = s_t.shape
    out = torch.empty_like(s_t)
    check(load().mcedm_swe_fv_step(_ptr(s_t), _ptr(out), B, T, X, half_dt, dx, _stream()), "swe_fv_step")
    return out


def swe_fv_unroll(ic: torch.Tensor, n_steps: int, half_dt: float, dx: float, gt: Optional[torch.Tensor] = None,
                  scale2: Optional[Sequence[float]] = None):
    """SweFvLoss.unroll_from_init on the initial rows ``ic`` (b, 1, x, 2) or (b, x, 2), fp32: ``out`` (b, n_steps + 1, x, 2) in one
    launch.  With ``gt`` (the shape of ``out``) and ``scale2 = (scale2_h, scale2_u)`` also the residual of unroll_loss,
    ``(out - gt) ** 2 / scale2``; returns ``(loss, out)`` then.  ``ic`` may be a view whose samples are strided (``pred[:, 0:1]``):
    it is read in place; only its rows must be dense."""
    if not ic.is_cuda:
        raise RuntimeError("libmcedm_hip needs device tensors (got a CPU tensor); there is no CPU fallback")
    if ic.dtype != torch.float32:
        raise RuntimeError(f"expected dtype {torch.float32}, got {ic.dtype}")
    rows = ic[:, 0] if ic.dim() == 4 else ic
    if rows.dim() != 3 or rows.shape[2] != 2 or (ic.dim() == 4 and ic.shape[1] != 1):
        raise RuntimeError(f"swe_fv_unroll: ic must be (b, 1, x, 2) or (b, x, 2), got {tuple(ic.shape)}")
    B, X, _ = rows.shape
    dense = rows.stride(2) == 1 and (X == 1 or rows.stride(1) == 2)
    if not dense or (B > 1 and rows.stride(0) < 2 * X):
        rows = rows.contiguous()
    if (gt is None) != (scale2 is None):
        raise RuntimeError("swe_fv_unroll: gt and scale2 go together")
    n_steps = int(n_steps)
    out = torch.empty((B, max(n_steps, 0) + 1, X, 2), dtype=torch.float32, device=ic.device)
    loss, s2h, s2u = None, 1.0, 1.0
    if gt is not None:
        if tuple(gt.shape) != tuple(out.shape):
            raise RuntimeError(f"swe_fv_unroll: gt must be {tuple(out.shape)}, got {tuple(gt.shape)}")
        loss, (s2h, s2u) = torch.empty_like(out), scale2
    stride = rows.stride(0) if B > 1 else 2 * X
    if B == 0:                               # an empty tensor has no pointer to pass
        return out if gt is None else (loss, out)
    check(load().mcedm_swe_fv_unroll(rows.data_ptr(), stride, _ptr(out), _ptr(gt), _ptr(loss), B, n_steps, X, half_dt, dx,
                                     float(s2h), float(s2u), _stream()), "swe_fv_unroll")
    return out if gt is None else (loss, out)


def swe_fv_residual(pred, gt, half_dt: float, dx: float, scale2_h: float, scale2_u: float, clamp: bool) -> torch.Tensor:
    B, T, X, _ = pred.shape
    out = torch.empty_like(pred)
    check(load().mcedm_swe_fv_residual(_ptr(pred), _ptr(gt), _ptr(out), B, T, X, half_dt, dx, scale2_h, scale2_u, int(clamp),
                                       _stream()), "swe_fv_residual")
    return out


def swe_fv_guidance(pred, gt, half_dt: float, dx: float, scale2_h: float, scale2_u: float) -> torch.Tensor:
    """SweFvLoss.forward(return_d=True): d mean(residual) / d pred on (b, t, x, 2) fp32 states."""
    B, T, X, _ = pred.shape
    out = torch.empty_like(pred)
    check(load().mcedm_swe_fv_guidance(_ptr(pred), _ptr(gt), _ptr(out), B, T, X, half_dt, dx, scale2_h, scale2_u, _stream()),
          "swe_fv_guidance")
    return out


def darcy_guidance(pred, two_dx: float, calc_prob: bool) -> torch.Tensor:
    B, S = pred.shape[0], pred.shape[1]
    out = torch.empty_like(pred)
    scratch = torch.empty(B * (S - 4) * (S - 4), dtype=torch.float32, device=pred.device)
    check(load().mcedm_darcy_guidance(_ptr(pred), _ptr(out), _ptr(scratch), B, S, two_dx, int(calc_prob), _stream()),
          "darcy_guidance")
    return out


def darcy_residual(pred, two_dx: float, denom: float, clamp: bool) -> torch.Tensor:
    B, S = pred.shape[0], pred.shape[1]
    out = torch.empty((B, S - 4, S - 4), dtype=torch.float32, device=pred.device)
    check(load().mcedm_darcy_residual(_ptr(pred), _ptr(out), B, S, two_dx, denom, int(clamp), _stream()), "darcy_residual")
    return out


def sqnorm(g: torch.Tensor, out: Optional[torch.Tensor] = None, scratch: Optional[torch.Tensor] = None) -> torch.Tensor:
    if out is None:
        out = torch.empty(1, dtype=torch.float64, device=g.device)
    scratch = reduce_scratch(g.device) if scratch is None else scratch
    check(load().mcedm_sqnorm(_ptr(g), g.numel(), _ptr(out, torch.float64), scratch.data_ptr(),
                              scratch.numel() * scratch.element_size(), _stream()), "sqnorm")
    return out


def adam_ema_step(param, grad, exp_avg, exp_avg_sq, ema, step, lr=2e-4, beta1=0.9, beta2=0.999, eps=1e-8,
                  weight_decay=0.0, sqnorm_t=None, max_norm=1.0, grad_scale=1.0, ema_beta=0.999):
    check(load().mcedm_adam_ema_step(_ptr(param), _ptr(grad), _ptr(exp_avg), _ptr(exp_avg_sq), _ptr(ema), param.numel(),
                                     lr, beta1, beta2, eps, weight_decay, _ptr(sqnorm_t, torch.float64), max_norm,
                                     grad_scale, ema_beta, int(step), _stream()), "adam_ema_step")


# ---- kernel-level ops (tests, per-kernel timing) ---------------------------------------------------
def _bind_ops() -> C.CDLL:
    """The loaded library; load() binds the kernel-level entries with every other one."""
    return load()


def prof_enable(on: bool) -> None:
    lib = load()
    check(lib.mcedm_prof_enable(int(on)), "prof_enable")


def prof_report() -> list:
    """Kernel-level timing rows collected since prof_enable(True) (synchronises the recorded events).  A row whose launcher chooses
    among kernels or template instantiations under one name also has "variants": {variant: launches}."""
    import json
    lib = load()
    buf = C.create_string_buffer(1 << 16)
    check(lib.mcedm_prof_report(buf, len(buf)), "prof_report")
    return json.loads(buf.value.decode())


def set_conv_tile(mt: int = 0, ph: int = 0, pw: int = 0) -> None:
    """Test hook: force the conv tile configuration; () restores the heuristic."""
    lib = _bind_ops()
    check(lib.mcedm_op_set_conv_tile(mt, ph, pw), "set_conv_tile")


# The process-wide form of the kernel switches, one set_<name>(enable=-1) each over mcedm_op_set_<name>: any integer, < 0 = not set (the
# plan's own choice aside, the environment decides).  Rows in the order of VARIANTS and of the table in csrc/switches.hpp: (name, docstring)
_SWITCH_SETTERS = (
    ("conv_wino", """Winograd F(2x2, 3x3) kernels in the network paths: 1 / 0; -1 = default (on).  Set before the workspace is laid out."""),
    ("conv_wino1", """Which Winograd kernel serves the 128-channel shapes: 1 = one wave per SIMD (conv_wino1.hip), 0 = two (conv_wino.hip);
    -1 = default (0: the one-wave kernel is 6-9 % slower).  Bit-identical results either way."""),
    ("conv_resident", """Input-resident conv kernels for <= 32 x 32 images: 1 / 0; -1 = default (on)."""),
    ("conv8", """Select the experimental 8-wave conv kernel (1 / 0; -1 = default)."""),
    ("attn_fused", """Single-launch attention block at 8 x 8 x 64 (inference): 1 / 0; -1 = default (on)."""),
    ("wgrad_wino", """Winograd F(3x3, 2x2) weight-gradient kernel (wgrad_wino.hip): 1 / 0 (direct split-K kernel everywhere); -1 = default (on)."""),
    ("conv1x1_reg", """Register-direct GEMM kernel for un-transformed 1x1 convs (conv1x1_reg.hip): 1 / 0 (conv_mfma_kernel); -1 = default (on)."""),
    ("conv_wino_fold", """The Winograd conv1 of an un-resampled decoder block computes the block's 1x1 skip projection in its epilogue (conv_wino.hip,
    the SKIP variant): 1 / 0 (a conv1x1_reg_kernel launch plus a residual read); -1 = default (on).  Same bits either way."""),
    ("conv_wino_upz", """The up-sampling Winograd convs skip the seven positions whose transformed input is exactly zero and stage their input at source
    resolution (conv_wino.hip, WinoUp): 1 / 0 (all sixteen positions); 2 = the positions alone, on the sixteen-position kernel's
    staging (A/B runs); -1 = default (on).  Same bits in every form."""),
    ("conv_wino_split", """The un-resampled 3x3 convs of images below 32 x 32 (the 16 x 16 level) run on the Winograd kernel with one 32-channel block per
    workgroup and the sixteen positions split over its waves (conv_wino.hip, WinoSplitCfg): 1 / 0 (the input-resident / tiled
    kernels); -1 = default (on).  An explicit set_conv_resident / set_conv_tile wins."""),
)


def _switch_setter(name: str, doc: str):
    def setter(enable: int = -1) -> None:
        check(getattr(_bind_ops(), "mcedm_op_set_" + name)(int(enable)), "set_" + name)
    setter.__name__ = setter.__qualname__ = "set_" + name
    setter.__doc__ = doc
    return setter


for _name, _doc in _SWITCH_SETTERS:
    globals()["set_" + _name] = _switch_setter(_name, _doc)


def set_conv_debug(buf: Optional[torch.Tensor] = None) -> None:
    """Per-workgroup debug records of the conv kernels (include/mcedm_hip.h, mcedm_op_set_conv_debug): buf is a device tensor of
    64-bit words, 16 per blockIdx.x workgroup of the launches that follow; the Winograd kernels put their tiles per workgroup
    into word 4.  None switches the records off.  The caller keeps buf alive, and large enough, until it has cleared the hook."""
    lib = _bind_ops()
    if buf is not None and (not buf.is_cuda or buf.element_size() != 8 or not buf.is_contiguous() or buf.numel() % 16):
        raise ValueError("set_conv_debug: buf must be a contiguous device tensor of 64-bit words, 16 per workgroup")
    check(lib.mcedm_op_set_conv_debug(buf.data_ptr() if buf is not None else None), "set_conv_debug")


RS_NONE, RS_UP, RS_DOWN, RS_S2 = 0, 1, 2, 3


def op_pack_conv(w: torch.Tensor, b: Optional[torch.Tensor], qkv_heads: int = 0, dgrad: bool = False):
    lib = _bind_ops()
    Cout, Cin, k, _ = w.shape
    rows, cols = (Cin, Cout) if dgrad else (Cout, Cin)
    n = lib.mcedm_op_conv_packed_floats(rows, cols, k)
    wpk = torch.empty(n, dtype=torch.float32, device=w.device)
    bpk = torch.zeros((Cout + 31) // 32 * 32, dtype=torch.float32, device=w.device) if b is not None else None
    check(lib.mcedm_op_pack_conv(_ptr(w), _ptr(b), Cout, Cin, k, qkv_heads, int(dgrad), _ptr(wpk), _ptr(bpk), _stream()),
          "op_pack_conv")
    return wpk, bpk


def op_gn_coef(xa, xb, gamma, beta, film=None, film_batch=0, film_stride=0, eps=1e-5, want_stats=False):
    lib = _bind_ops()
    B, Ca = xa.shape[:2]
    Cb = xb.shape[1] if xb is not None else 0
    HW = xa[0, 0].numel()
    Ct = Ca + Cb
    coef = torch.empty((B, Ct, 4), dtype=torch.float32, device=xa.device)
    stats = torch.empty((B, min(32, Ct // 4), 2), dtype=torch.float32, device=xa.device) if want_stats else None
    check(lib.mcedm_op_gn_coef(_ptr(xa), _ptr(xb), Ca, Cb, B, HW, _ptr(gamma), _ptr(beta), _ptr(film), film_batch,
                               film_stride, eps, _ptr(coef), _ptr(stats), _stream()), "op_gn_coef")
    return (coef, stats) if want_stats else coef


def op_conv(xa, xb, wpk, bias_pk, Cout, k, coef=None, coef_batch=1, act=0, resample=RS_NONE, res=None,
            res_mode=RS_NONE, out=None, bias_batch=0):
    """bias_batch != 0: bias_pk is [B, bias_batch], a (packed) row per sample (mcedm_op_conv_bias_batch)."""
    lib = _bind_ops()
    B, Ca, Hs, Ws = xa.shape
    Cb = xb.shape[1] if xb is not None else 0
    H, W = (Hs * 2, Ws * 2) if resample == RS_UP else ((Hs // 2, Ws // 2) if resample in (RS_DOWN, RS_S2) else (Hs, Ws))
    if out is None:
        out = torch.empty((B, Cout, H, W), dtype=torch.float32, device=xa.device)
    if bias_batch:
        if bias_pk is None or bias_pk.numel() < (B - 1) * bias_batch + Cout:
            raise RuntimeError(f"op_conv: bias_batch={bias_batch} needs a bias of {B} rows")
        check(lib.mcedm_op_conv_bias_batch(_ptr(xa), _ptr(xb), Ca, Cb, _ptr(coef), coef_batch, act, resample, Hs, Ws, H, W, _ptr(wpk),
                                           _ptr(bias_pk), int(bias_batch), _ptr(res), res_mode, _ptr(out), Cout, B, k, _stream()),
              "op_conv_bias_batch")
        return out
    check(lib.mcedm_op_conv(_ptr(xa), _ptr(xb), Ca, Cb, _ptr(coef), coef_batch, act, resample, Hs, Ws, H, W, _ptr(wpk),
                            _ptr(bias_pk), _ptr(res), res_mode, _ptr(out), Cout, B, k, _stream()), "op_conv")
    return out


def op_pack_conv_wino(w: torch.Tensor, dgrad: bool = False) -> torch.Tensor:
    """[Cout, Cin, 3, 3] -> the Winograd F(2x2, 3x3) weight table of mcedm_op_conv_wino.  dgrad: the table of the data gradient
    instead (channels transposed, taps mirrored): op_conv_wino(dy, None, table, None, Cin) is then d/dx of the forward conv."""
    lib = _bind_ops()
    Cout, Cin = w.shape[:2]
    if dgrad:
        wino = torch.empty(lib.mcedm_op_conv_wino_packed_floats(Cin, Cout), dtype=torch.float32, device=w.device)
        check(lib.mcedm_op_pack_conv_wino_dgrad(_ptr(w), Cout, Cin, _ptr(wino), _stream()), "op_pack_conv_wino_dgrad")
        return wino
    wino = torch.empty(lib.mcedm_op_conv_wino_packed_floats(Cout, Cin), dtype=torch.float32, device=w.device)
    check(lib.mcedm_op_pack_conv_wino(_ptr(w), Cout, Cin, _ptr(wino), _stream()), "op_pack_conv_wino")
    return wino


def op_conv_wino(xa, xb, wino, bias, Cout, coef=None, coef_batch=1, act=0, resample=RS_NONE, res=None, res_mode=RS_NONE,
                 out=None, want_sums=False, bias_batch=0):
    """want_sums: -> (out, the fused GroupNorm records of out as a plan's convs write them).  bias_batch != 0 (with want_sums):
    bias is [B, bias_batch], a row per sample (mcedm_op_conv_wino_sums_bias_batch)."""
    lib = _bind_ops()
    B, Ca, Hs, Ws = xa.shape
    Cb = xb.shape[1] if xb is not None else 0
    H, W = (Hs * 2, Ws * 2) if resample == RS_UP else (Hs, Ws)
    if out is None:
        out = torch.empty((B, Cout, H, W), dtype=torch.float32, device=xa.device)
    if bias_batch and (not want_sums or bias is None or bias.numel() < (B - 1) * bias_batch + Cout):
        raise RuntimeError(f"op_conv_wino: bias_batch={bias_batch} goes with want_sums and a bias of {B} rows")
    if want_sums:
        gsum = torch.zeros(B * ((H + 3) // 4) * ((W + 7) // 8) * ((Cout + 3) // 4) * 2, dtype=torch.float32, device=xa.device)
        if bias_batch:
            check(lib.mcedm_op_conv_wino_sums_bias_batch(_ptr(xa), _ptr(xb), Ca, Cb, _ptr(coef), coef_batch, act, resample, H, W,
                                                         _ptr(wino), _ptr(bias), int(bias_batch), _ptr(res), res_mode, _ptr(out),
                                                         _ptr(gsum), Cout, B, _stream()), "op_conv_wino_sums_bias_batch")
            return out, gsum
        check(lib.mcedm_op_conv_wino_sums(_ptr(xa), _ptr(xb), Ca, Cb, _ptr(coef), coef_batch, act, resample, H, W, _ptr(wino),
                                          _ptr(bias), _ptr(res), res_mode, _ptr(out), _ptr(gsum), Cout, B, _stream()), "op_conv_wino_sums")
        return out, gsum
    check(lib.mcedm_op_conv_wino(_ptr(xa), _ptr(xb), Ca, Cb, _ptr(coef), coef_batch, act, resample, H, W, _ptr(wino),
                                 _ptr(bias), _ptr(res), res_mode, _ptr(out), Cout, B, _stream()), "op_conv_wino")
    return out


def op_conv_wino_split(xa, xb, wino, bias, Cout, coef=None, coef_batch=1, act=0, res=None, res_mode=RS_NONE, out=None, want_sums=False):
    """op_conv_wino on the split variant of the kernel (mcedm_op_conv_wino_split / _sums): un-resampled, images below 32 x 32,
    Cout % 32 == 0.  want_sums: -> (out, the fused GroupNorm records of out)."""
    lib = _bind_ops()
    B, Ca, H, W = xa.shape
    Cb = xb.shape[1] if xb is not None else 0
    if out is None:
        out = torch.empty((B, Cout, H, W), dtype=torch.float32, device=xa.device)
    if want_sums:
        gsum = torch.zeros(B * ((H + 3) // 4) * ((W + 7) // 8) * ((Cout + 3) // 4) * 2, dtype=torch.float32, device=xa.device)
        check(lib.mcedm_op_conv_wino_split_sums(_ptr(xa), _ptr(xb), Ca, Cb, _ptr(coef), coef_batch, act, H, W, _ptr(wino), _ptr(bias),
                                                _ptr(res), res_mode, _ptr(out), _ptr(gsum), Cout, B, _stream()), "op_conv_wino_split_sums")
        return out, gsum
    check(lib.mcedm_op_conv_wino_split(_ptr(xa), _ptr(xb), Ca, Cb, _ptr(coef), coef_batch, act, H, W, _ptr(wino), _ptr(bias), _ptr(res),
                                       res_mode, _ptr(out), Cout, B, _stream()), "op_conv_wino_split")
    return out


def op_pack_conv_frag(w: torch.Tensor) -> torch.Tensor:
    """[Cout, Cin, 1, 1] -> the 1x1 weights in the MFMA-fragment order op_conv_skip's sk_wfrag expects."""
    lib = _bind_ops()
    Cout, Cin = w.shape[:2]
    wfrag = torch.empty((Cout + 31) // 32 * 32 * ((Cin + 7) // 8 * 8), dtype=torch.float32, device=w.device)
    check(lib.mcedm_op_pack_conv_frag(_ptr(w), Cout, Cin, _ptr(wfrag), _stream()), "op_pack_conv_frag")
    return wfrag


def op_conv_skip(x, wpk, wino, bias, Cout, coef=None, act=1, res=None, sk_xa=None, sk_xb=None, sk_wpk=None, sk_wfrag=None,
                 sk_bias=None, want_sums=False):
    """conv1 of a decoder block through the dispatcher (mcedm_op_conv_skip): 3x3 conv of act(coef(x)) plus either the residual
    res or the folded 1x1 projection of cat(sk_xa, sk_xb).  -> out, or (out, the fused GroupNorm records) with want_sums."""
    lib = _bind_ops()
    B, Cin, H, W = x.shape
    out = torch.empty((B, Cout, H, W), dtype=torch.float32, device=x.device)
    gsum = torch.zeros(B * ((H + 3) // 4) * ((W + 7) // 8) * ((Cout + 3) // 4) * 2, dtype=torch.float32, device=x.device) if want_sums else None
    check(lib.mcedm_op_conv_skip(_ptr(x), Cin, _ptr(coef), act, H, W, _ptr(wpk), _ptr(wino), _ptr(bias), _ptr(res), _ptr(sk_xa), _ptr(sk_xb),
                                 sk_xa.shape[1] if sk_xa is not None else 0, sk_xb.shape[1] if sk_xb is not None else 0, _ptr(sk_wpk),
                                 _ptr(sk_wfrag), _ptr(sk_bias), _ptr(out), _ptr(gsum), Cout, B, _stream()), "op_conv_skip")
    return (out, gsum) if want_sums else out


def _conv_hw(xa, resample):
    Hs, Ws = xa.shape[2:]
    H, W = (Hs * 2, Ws * 2) if resample == RS_UP else ((Hs // 2, Ws // 2) if resample in (RS_DOWN, RS_S2) else (Hs, Ws))
    return Hs, Ws, H, W


def _tiling_arg(t):
    return None if t is None else (C.c_int * 5)(*[int(v) for v in t])


def op_conv_sums(xa, xb, wpk, bias_pk, Cout, k, rc=4, wino=None, coef=None, coef_batch=1, act=0, resample=RS_NONE, res=None,
                 res_mode=RS_NONE, bias_batch=0):
    """op_conv through the dispatcher with the fused GroupNorm records of its output (mcedm_op_conv_sums): rc channels per record
    (4 or 2); wino: op_pack_conv_wino's table, with which the Winograd kernels may take the launch as in a plan.
    -> (out, records [B, tiles, Cout / rc, 2] = (sum, M2), tiling = (tiles, tiles_x, ph, pw, rc) as the launcher chose it).
    The table is filled with NaN before the launch: a record the kernel does not write shows."""
    lib = _bind_ops()
    B, Ca = xa.shape[:2]
    Cb = xb.shape[1] if xb is not None else 0
    Hs, Ws, H, W = _conv_hw(xa, resample)
    out = torch.empty((B, Cout, H, W), dtype=torch.float32, device=xa.device)
    nrec = -(-Cout // (2 if rc == 2 else 4))
    gsum = torch.full((B * ((H + 3) // 4) * ((W + 7) // 8) * nrec * 2,), float("nan"), dtype=torch.float32, device=xa.device)
    tiling = (C.c_int * 5)()
    check(lib.mcedm_op_conv_sums(_ptr(xa), _ptr(xb), Ca, Cb, _ptr(coef), coef_batch, act, resample, Hs, Ws, H, W, _ptr(wpk), _ptr(wino),
                                 _ptr(bias_pk), int(bias_batch), _ptr(res), res_mode, _ptr(out), Cout, B, k, _ptr(gsum), int(rc), tiling,
                                 _stream()), "op_conv_sums")
    tiling = tuple(tiling)
    if tiling[0] > ((H + 3) // 4) * ((W + 7) // 8):
        raise RuntimeError(f"op_conv_sums: the launcher reports {tiling[0]} tiles, beyond the table")
    return out, gsum[:B * tiling[0] * nrec * 2].view(B, tiling[0], nrec, 2), tiling


def op_gn_coef_from_sums(suma, tiling_a, Ca, H, W, groups, gamma, beta, sumb=None, tiling_b=None, Cb=0, film=None, film_batch=0,
                         film_stride=0, eps=1e-5):
    """gn_coef_from_sums_kernel on records alone (mcedm_op_gn_coef_from_sums) -> (coef [B, Ca + Cb, 4], stats [B, groups, 2])."""
    lib = _bind_ops()
    B = suma.shape[0]
    coef = torch.empty((B, Ca + Cb, 4), dtype=torch.float32, device=suma.device)
    stats = torch.empty((B, groups, 2), dtype=torch.float32, device=suma.device)
    check(lib.mcedm_op_gn_coef_from_sums(_ptr(suma), _ptr(sumb), _tiling_arg(tiling_a), _tiling_arg(tiling_b), Ca, Cb, B, H, W, groups,
                                         _ptr(gamma), _ptr(beta), _ptr(film), film_batch, film_stride, eps, _ptr(coef), _ptr(stats),
                                         _stream()), "op_gn_coef_from_sums")
    return coef, stats


def op_conv_gn(xa, xb, suma, tiling_a, groups, gamma, beta, wpk, bias_pk, Cout, k, sumb=None, tiling_b=None, film=None, film_batch=0,
               film_stride=0, eps=1e-5, act=1, wino=None, resample=RS_NONE, res=None, res_mode=RS_NONE):
    """op_conv whose GroupNorm (+ FiLM) rows the kernel derives from the records of cat(xa, xb) (mcedm_op_conv_gn)."""
    lib = _bind_ops()
    B, Ca = xa.shape[:2]
    Cb = xb.shape[1] if xb is not None else 0
    Hs, Ws, H, W = _conv_hw(xa, resample)
    out = torch.empty((B, Cout, H, W), dtype=torch.float32, device=xa.device)
    check(lib.mcedm_op_conv_gn(_ptr(xa), _ptr(xb), Ca, Cb, _ptr(suma), _ptr(sumb), _tiling_arg(tiling_a), _tiling_arg(tiling_b), groups,
                               _ptr(gamma), _ptr(beta), _ptr(film), film_batch, film_stride, eps, act, resample, Hs, Ws, H, W, _ptr(wpk),
                               _ptr(wino), _ptr(bias_pk), _ptr(res), res_mode, _ptr(out), Cout, B, k, _stream()), "op_conv_gn")
    return out


def op_embedding(labels, w0, b0, w1, b1, waff, baff):
    """-> (emb [n, ch], film [n, rows]): sigma-embedding MLP + the concatenated per-block affine rows (K6)."""
    lib = _bind_ops()
    n, ch, rows = labels.numel(), w0.shape[0], waff.shape[0]
    freqs = torch.empty(ch // 2, dtype=torch.float32, device=labels.device)
    emb = torch.empty((n, ch), dtype=torch.float32, device=labels.device)
    film = torch.empty((n, rows), dtype=torch.float32, device=labels.device)
    check(lib.mcedm_op_embedding(_ptr(labels), n, ch, _ptr(w0), _ptr(b0), _ptr(w1), _ptr(b1), _ptr(waff), _ptr(baff), rows,
                                 _ptr(freqs), _ptr(emb), _ptr(film), _stream()), "op_embedding")
    return emb, film


def op_attention(qkv: torch.Tensor, heads: int) -> torch.Tensor:
    """qkv [B, heads*3*64, H, W] in packed (head, {q,k,v}, c) channel order -> [B, heads*64, H, W]."""
    lib = _bind_ops()
    B, C3, H, W = qkv.shape
    out = torch.empty((B, C3 // 3, H, W), dtype=torch.float32, device=qkv.device)
    check(lib.mcedm_op_attention(_ptr(qkv), _ptr(out), B, heads, H * W, _stream()), "op_attention")
    return out


def op_attn_block(y, gamma, beta, wq_pk, bq_pk, wp_pk, bp_pk, eps=1e-5, want_sums=False):
    """The fused 8 x 8 x 64 attention block (attn_block64_kernel) on its own: z = proj(attention(qkv(group_norm(y)))) + y for
    y [B, 64, 8, 8].  wq_pk, bq_pk = op_pack_conv(qkv.weight, qkv.bias, qkv_heads=1); wp_pk, bp_pk = op_pack_conv(proj.weight,
    proj.bias).  want_sums: -> (z, gsum [B, 16, 2]), the fused GroupNorm records (sum, M2) of z per 4-channel group."""
    lib = _bind_ops()
    if y.dim() != 4 or tuple(y.shape[1:]) != (64, 8, 8):
        raise RuntimeError(f"op_attn_block: y must be [B, 64, 8, 8], got {tuple(y.shape)}")
    B = y.shape[0]
    z = torch.empty_like(y)
    gsum = torch.zeros((B, 16, 2), dtype=torch.float32, device=y.device) if want_sums else None
    check(lib.mcedm_op_attn_block64(_ptr(y), _ptr(gamma), _ptr(beta), eps, _ptr(wq_pk), _ptr(bq_pk), _ptr(wp_pk), _ptr(bp_pk),
                                    _ptr(z), _ptr(gsum), B, _stream()), "op_attn_block64")
    return (z, gsum) if want_sums else z


def op_conv_wgrad(dy, xa, xb, k, coef=None, coef_batch=1, act=0, resample=RS_NONE, qkv_heads=0):
    """-> (dw [Cout, Cin, k, k], db [Cout])"""
    lib = _bind_ops()
    B, Cout, H, W = dy.shape
    Ca, Hs, Ws = xa.shape[1], xa.shape[2], xa.shape[3]
    Cb = xb.shape[1] if xb is not None else 0
    Cin = Ca + Cb
    scratch = torch.empty(lib.mcedm_op_wgrad_scratch_floats(Cout, Cin, k, B, H, W), dtype=torch.float32, device=dy.device)
    dw = torch.empty((Cout, Cin, k, k), dtype=torch.float32, device=dy.device)
    db = torch.empty(Cout, dtype=torch.float32, device=dy.device)
    check(lib.mcedm_op_conv_wgrad(_ptr(dy), _ptr(xa), _ptr(xb), Ca, Cb, _ptr(coef), coef_batch, act, resample, Hs, Ws, H,
                                  W, Cout, B, k, qkv_heads, _ptr(scratch), _ptr(dw), _ptr(db), _stream()), "op_conv_wgrad")
    return dw, db


def op_gn_bwd(dact, xa, xb, coef, stats, gamma, beta, film=None, film_batch=0, film_stride=0, act=1,
              resample=RS_NONE, add=None, add_mode=0, dx_init=None, sync=None):
    """-> (dxa, dxb, dgamma, dbeta, dfilm or None); dx_init (tuple) makes the call accumulate into copies of it.  sync: a zeroed
    int32 tensor of GN_SYNC_WORDS * B * groups words (mcedm_op_gn_bwd_sync: slabs split over workgroups keep their pieces in LDS)."""
    lib = _bind_ops()
    B, Ca, Hs, Ws = xa.shape
    Cb = xb.shape[1] if xb is not None else 0
    Ct = Ca + Cb
    dxa = dx_init[0].clone() if dx_init else torch.empty_like(xa)
    dxb = (dx_init[1].clone() if dx_init else torch.empty_like(xb)) if xb is not None else None
    ab = torch.empty((B, Ct, 2), dtype=torch.float32, device=xa.device)
    dg, dbt = torch.empty(Ct, device=xa.device), torch.empty(Ct, device=xa.device)
    dfilm = torch.zeros((B if film_batch else 1, 2 * Ct), dtype=torch.float32, device=xa.device) if film is not None else None
    args = (_ptr(dact), resample, _ptr(xa), _ptr(xb), Ca, Cb, Hs, Ws, B, _ptr(coef), _ptr(stats),
            _ptr(gamma), _ptr(beta), _ptr(film), film_batch, film_stride, act, _ptr(dxa), _ptr(dxb),
            int(dx_init is not None), _ptr(add), add_mode, _ptr(ab), _ptr(dg), _ptr(dbt), _ptr(dfilm), 2 * Ct)
    if sync is not None:
        if sync.dtype != torch.int32 or sync.numel() < GN_SYNC_WORDS * B * min(32, Ct // 4) or not sync.is_cuda:
            raise ValueError("op_gn_bwd: sync must be a device int32 tensor of at least GN_SYNC_WORDS * B * groups zeros")
        check(lib.mcedm_op_gn_bwd_sync(*args, _ptr(sync, torch.int32), _stream()), "op_gn_bwd_sync")
    else:
        check(lib.mcedm_op_gn_bwd(*args, _stream()), "op_gn_bwd")
    return dxa, dxb, dg, dbt, dfilm


def op_attention_bwd(qkv, a, da, heads, out=None):
    """-> dqkv; out: a caller-owned contiguous tensor of qkv's shape, dtype and device to write it into (every element is written)."""
    lib = _bind_ops()
    B, C3, H, W = qkv.shape
    dqkv = torch.empty_like(qkv) if out is None else out
    if dqkv.shape != qkv.shape or dqkv.device != qkv.device:
        raise ValueError("op_attention_bwd: out must have qkv's shape and device")
    lse = torch.empty(B * heads * H * W * 2, dtype=torch.float32, device=qkv.device)
    check(lib.mcedm_op_attention_bwd(_ptr(qkv), _ptr(a), _ptr(da), _ptr(dqkv), _ptr(lse), B, heads, H * W, _stream()),
          "op_attention_bwd")
    return dqkv


def op_ddim_cond_step(xt, F, s0, s1, sa_next, c2, Fu=None, w=0.0, noise=None, c1=0.0, condp=None, condp_u=None, cond_channels=0,
                      xs=None, t_xs=0, x0s=None, t_x0=0, rng_seed=None, draw=0, dx=None, gw=None):
    """One elementwise step of the conditional DDIM sampler (mcedm_op_ddim_cond_step) -> xt_next.  x0 is written into channels
    [cond_channels, cond_channels + C) of condp / condp_u and into slot t_x0 of x0s, xt_next into slot t_xs of xs ('b t h w c').
    rng_seed (int64 [1] on the device) with draw: the kernel generates the uniform noise itself (mcedm_op_ddim_cond_step_rng).
    dx [B, 1, H, W] and gw (or gw alone, dx None): mcedm_op_ddim_cond_step_guided, both noise forms in its one signature, with the
    PDE-guidance term et -= gw * dx."""
    lib = _bind_ops()
    B, Cc, H, W = xt.shape
    xt_next = torch.empty_like(xt)
    args = (float(w), s0, s1, sa_next, c1, c2, _ptr(xt_next), _ptr(condp), _ptr(condp_u), int(cond_channels),
            0 if condp is None else condp.shape[1], B, Cc, H, W, _ptr(xs), 0 if xs is None else xs.shape[1], int(t_xs), _ptr(x0s),
            0 if x0s is None else x0s.shape[1], int(t_x0))
    if dx is not None or gw is not None:
        if dx is not None and tuple(dx.shape) != (B, 1, H, W):
            raise RuntimeError(f"op_ddim_cond_step: dx must be {(B, 1, H, W)}, got {tuple(dx.shape)}")
        seed = None if rng_seed is None else _seed_ptr(rng_seed, xt.device, "op_ddim_cond_step")
        check(lib.mcedm_op_ddim_cond_step_guided(_ptr(xt), _ptr(F), _ptr(Fu), _ptr(noise), seed, int(draw), _ptr(dx), float(gw or 0.0),
                                                 *args, _stream()), "op_ddim_cond_step_guided")
        return xt_next
    if rng_seed is not None:
        if noise is not None:
            raise RuntimeError("op_ddim_cond_step: give noise or rng_seed, not both")
        check(lib.mcedm_op_ddim_cond_step_rng(_ptr(xt), _ptr(F), _ptr(Fu), _seed_ptr(rng_seed, xt.device, "op_ddim_cond_step"),
                                              int(draw), *args, _stream()), "op_ddim_cond_step_rng")
        return xt_next
    check(lib.mcedm_op_ddim_cond_step(_ptr(xt), _ptr(F), _ptr(Fu), _ptr(noise), *args, _stream()), "op_ddim_cond_step")
    return xt_next


def op_dropout_act(h, p, rng_seed, draw, coef=None, coef_batch=1):
    """out = mask * s * silu((h - mean) * scale + offset) (mcedm_op_dropout_act): h [B, C, H, W]; coef [B or 1, C, 4] rows (mean, scale,
    offset, pad) or None (identity); the mask and s = 1 / (1 - p) of draw ``draw`` of the uniform generator keyed by rng_seed
    (int64 [1] on the device), as mcedm_unet_plan_set_dropout states them."""
    lib = _bind_ops()
    B, Cc, H, W = h.shape
    out = torch.empty_like(h)
    check(lib.mcedm_op_dropout_act(_ptr(h), _ptr(coef), int(coef_batch), _ptr(out), B, Cc, H, W, float(p),
                                   _seed_ptr(rng_seed, h.device, "op_dropout_act"), int(draw), _stream()), "op_dropout_act")
    return out


def op_dropout_scale(g, p, rng_seed, draw):
    """g <- mask * s * g in place (mcedm_op_dropout_scale), g [B, C, H, W]; returns g."""
    lib = _bind_ops()
    B, Cc, H, W = g.shape
    check(lib.mcedm_op_dropout_scale(_ptr(g), B, Cc, H, W, float(p), _seed_ptr(rng_seed, g.device, "op_dropout_scale"), int(draw),
                                     _stream()), "op_dropout_scale")
    return g
