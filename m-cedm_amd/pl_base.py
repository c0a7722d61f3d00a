"""What the four Lightning drop-ins (``mcedm.PlMcedm``, ``ddim.PlDdim`` / ``PlCondEdm`` / ``PlCondDdim``) share:

  * the Lightning fallback ``_Base``, ``DotDict``, ``Normalizer`` and the small helpers (``_nchw``, ``_opt``, ``_beta_schedule``,
    the metric functions ``masked_l1`` / ``l1`` / ``correlation``);
  * ``_TrainLoss``, the one autograd Function of the training steps (generation guard, flat gradient buffer);
  * ``_PlBase``: constructor helpers, ``setup``, the data transforms, the optimiser hooks, ``_net`` / ``_grad_views``, the
    graph-replay scaffolding of the samplers and the host-side metric bookkeeping of the evaluation loops.

Everything model-specific (constructor checks, ``training_step``, ``get_denoised``, ``sample_edm``) stays with its class.
"""
from __future__ import annotations

import math
import os

import numpy as np
import torch
from torch import nn

from . import lib as _lib
from .adm_blocks import EmaModel
from .pde_loss import get_pde_loss_function

try:  # Lightning is the reference's runtime; the build/test containers do not ship it
    import pytorch_lightning as pl
    _Base = pl.LightningModule
except Exception:  # pragma: no cover - exercised where Lightning is absent
    class _Base(nn.Module):
        """Minimal stand-in so the module is usable (and testable) without pytorch_lightning."""
        current_epoch = 0

        def save_hyperparameters(self, *a, **k):
            pass

        def log(self, *a, **k):
            pass

        # Lightning's defaults for the two hooks the drop-in overrides (pytorch_lightning/core/module.py): the optimiser step runs
        # the closure (zero_grad + training_step + backward), gradient clipping is clip_grad_norm_ on the optimiser's parameters
        def optimizer_step(self, epoch=None, batch_idx=None, optimizer=None, optimizer_idx=0, optimizer_closure=None, *a, **k):
            optimizer.step(closure=optimizer_closure)

        def clip_gradients(self, optimizer, gradient_clip_val=None, gradient_clip_algorithm=None):
            if gradient_clip_val is None or gradient_clip_val <= 0:
                return
            params = [p for g in optimizer.param_groups for p in g["params"]]
            if gradient_clip_algorithm in (None, "norm"):
                torch.nn.utils.clip_grad_norm_(params, gradient_clip_val)
            else:
                torch.nn.utils.clip_grad_value_(params, gradient_clip_val)


class DotDict(dict):
    __getattr__ = dict.__getitem__
    __setattr__ = dict.__setitem__
    __delattr__ = dict.__delitem__


class Normalizer(nn.Module):
    """(x - subtract) / divide and its inverse; stats travel as buffers (models/normalizer.py:5-29)."""

    def __init__(self, stats_shape=()):
        super().__init__()
        self.register_buffer("subtract", torch.zeros(stats_shape))
        self.register_buffer("divide", torch.ones(stats_shape))

    def set_stats(self, subtract, divide):
        self.subtract = torch.as_tensor(subtract)
        self.divide = torch.as_tensor(divide)

    def forward(self, x, inverse=False):
        if inverse:
            return x * self.divide.to(x.device) + self.subtract.to(x.device)
        return (x - self.subtract.to(x.device)) / self.divide.to(x.device)


def _nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def _opt(cfg, name, default):
    """cfg.<name> if present (DictConfig, attribute dicts whose __getattr__ raises KeyError, plain objects)."""
    try:
        return getattr(cfg, name)
    except (AttributeError, KeyError):
        return default


def _beta_schedule(kind, beta_start, beta_end, n):
    """models/ddim_blocks.py:473-505."""
    if kind == "quad":
        b = np.linspace(beta_start ** 0.5, beta_end ** 0.5, n, dtype=np.float64) ** 2
    elif kind == "linear":
        b = np.linspace(beta_start, beta_end, n, dtype=np.float64)
    elif kind == "const":
        b = beta_end * np.ones(n, dtype=np.float64)
    elif kind == "jsd":
        b = 1.0 / np.linspace(n, 1, n, dtype=np.float64)
    elif kind == "sigmoid":
        b = 1 / (np.exp(-np.linspace(-6, 6, n)) + 1) * (beta_end - beta_start) + beta_start
    else:
        raise NotImplementedError(kind)
    return torch.from_numpy(b).float()


def _ddim_sampler_params():
    """The sampler of a config without one (models/mcedm.py:86-92, models/ddim.py:80-86)."""
    return DotDict(type="ddim", timesteps=50, skip_type="uniform", eta=0.0, n_samples=1, n_repeat=5, n_time_h=128, n_time_u=0)


# ---- metrics (models/losses.py) ----------------------------------------------------------------------------------------
def masked_l1(pred, target, mask, loss_dim=None):
    """MaskedLoss('l1') of models/losses.py:62-78: sum |pred*m - target*m| / sum(m)."""
    pred, target = pred * mask, target * mask
    if loss_dim is not None:
        pred, target, mask = pred[..., loss_dim], target[..., loss_dim], mask[..., loss_dim]
    return (pred - target).abs().sum() / mask.sum()


def l1(a, b):
    """nn.L1Loss() (mean); an empty slice gives nan like the reference's own call does."""
    return (a - b).abs().mean()


def correlation(pred, target):
    """CorrelationLoss(reduction='none'), models/losses.py:93-124: per-channel Pearson correlation over the grid, averaged
    over the batch."""
    p = pred.reshape(pred.shape[0], -1, pred.shape[-1])
    t = target.reshape(target.shape[0], -1, target.shape[-1])
    pc, tc = p - p.mean(dim=1, keepdim=True), t - t.mean(dim=1, keepdim=True)
    den = ((pc * pc).sum(dim=1) * (tc * tc).sum(dim=1)).sqrt()
    den = den + (den == 0) * 1e-7
    return ((tc * pc).sum(dim=1) / den).mean(dim=0)


class _TrainLoss(torch.autograd.Function):
    """The scalar training loss of one module, forward and backward both in the HIP library.  ``run()`` is the variant's
    forward + loss: it returns (loss, run_backward) with ``run_backward(grads)`` writing the parameter gradients of the
    UNSCALED loss into the views ``grads``.  Parameters enter as inputs so that Lightning's automatic optimisation and DDP see
    ordinary .grad tensors."""

    @staticmethod
    def forward(ctx, module, run, *params):
        loss, ctx.run_backward = run()
        # the activations of THIS forward live in the module's single training workspace until its backward runs
        module._train_generation += 1
        ctx.module, ctx.generation = module, module._train_generation
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        module = ctx.module
        if ctx.generation != module._train_generation:
            raise RuntimeError("training_step: another training forward overwrote this one's activations before its "
                               "backward ran (one outstanding forward per module; run backward before the next forward)")
        params = list(module.model.parameters())
        ctx.run_backward(module._grad_views(params))
        # one scale of the flat buffer into a FRESH tensor (autograd may keep the returned views as .grad, so they
        # must not alias the buffer the next backward overwrites) instead of one multiply per parameter
        flat = module._grad_buf * g.to(torch.float32)
        out, off = [], 0
        for p in params:
            out.append(flat[off:off + p.numel()].view(p.shape))
            off += p.numel()
        return (None, None) + tuple(out)


class _PlBase(_Base):
    """Constructor helpers, configuration hooks and host-side bookkeeping common to the four drop-ins."""

    # ---- constructor helpers ----------------------------------------------------------------------------------------
    def _register_schedule(self, hparams):
        """The DDPM schedule buffers ``betas`` / ``logvar`` of PlDdim.__init__ (models/ddim.py:22-30)."""
        m, df = hparams.model, hparams.diffusion
        betas = _beta_schedule(df.beta_schedule, df.beta_start, df.beta_end, df.num_diffusion_timesteps)
        acp = (1.0 - betas).cumprod(dim=0)
        post_var = betas * (1.0 - torch.cat([torch.ones(1), acp[:-1]])) / (1.0 - acp)
        self.model_var_type = m.var_type
        self.register_buffer("betas", betas)
        self.num_timesteps = betas.shape[0]
        if m.var_type == "fixedlarge":
            self.register_buffer("logvar", betas.log())
        elif m.var_type == "fixedsmall":
            self.register_buffer("logvar", post_var.clamp(min=1e-20).log())

    def _init_common(self, hparams, n_input, n_target, default_sampler=_ddim_sampler_params):
        """Everything after ``model`` / ``ema_model``: normalisers over n_input / n_target channels, data flags, optimiser
        fields, samplers, the default PDE loss (models/mcedm.py:82-84, models/ddim.py:76-78) and the module's workspaces."""
        o, d = hparams.optimization, hparams.data
        self.normalization, self.rescaled = d.normalization, d.rescaled
        self.uniform_dequantization, self.gaussian_dequantization = d.uniform_dequantization, d.gaussian_dequantization
        self.normalizer_input = Normalizer((n_input,) if n_input > 1 else ())
        self.normalizer_target = Normalizer((n_target,) if n_target > 1 else ())
        self.optimizer, self.lr, self.weight_decay = o.optimizer, o.lr, o.weight_decay
        self.beta1, self.amsgrad, self.eps = o.beta1, o.amsgrad, o.eps
        sp = hparams.get("sampler", None)
        self.sparams = self.test_sparams = default_sampler() if sp is None else sp
        self.set_pde_loss_function(system="swe", flip_xy=False)
        self._train_ws, self._sample_ws = _lib.Workspace(), _lib.Workspace()
        self._grad_buf, self._train_generation = None, 0
        self._graphs = {}

    # ---- configuration hooks (same names as the reference) ----------------------------------------------------------
    def set_pde_loss_function(self, system, flip_xy):
        """models/mcedm.py:100-104, models/ddim.py:97-101.  The residuals and their guidance gradients run on the device
        (m-cedm_amd/pde_loss.py -> csrc/pde.hip, bit-identical to models/pde_loss.py)."""
        self.pde_loss, self.pde_loss_simulator = get_pde_loss_function(system, flip_xy)

    def setup(self, stage: str = None) -> None:
        if stage == "fit":
            st = self.trainer.datamodule.get_norm_stats()
            key = ("min", "min_max") if self.normalization == "min_max" else ("mean", "std")
            self.normalizer_input.set_stats(st[f"input_{key[0]}"], st[f"input_{key[1]}"])
            self.normalizer_target.set_stats(st[f"target_{key[0]}"], st[f"target_{key[1]}"])

    def configure_optimizers(self):
        """models/mcedm.py:139-161.  ``optimizer: Adam`` on the device returns ``optim.FusedAdamEma`` -- a torch.optim.Optimizer
        over flat buffers whose ``step()`` is the fused clip + Adam + EMA kernels (K11), state_dict in torch.optim.Adam form;
        ``MCEDM_FUSED_OPT=0`` (or amsgrad, or a module still on the CPU) keeps plain ``torch.optim.Adam``."""
        self._fused_opt = None
        if self.optimizer == "Adam":
            p0 = next(self.model.parameters())
            if os.environ.get("MCEDM_FUSED_OPT", "1") != "0" and p0.is_cuda and not self.amsgrad:
                from .optim import FusedAdamEma
                ema = self.ema_model.ma_model if self.ema_model is not None else None
                opt = FusedAdamEma(self.model, ema, lr=self.lr, betas=(self.beta1, 0.999), eps=self.eps,
                                   weight_decay=self.weight_decay, ema_beta=self.ema_model.beta if ema is not None else 0.999)
                self._fused_opt = opt
                return {"optimizer": opt}
            opt = torch.optim.Adam(self.model.parameters(), lr=self.lr, weight_decay=self.weight_decay,
                                   betas=(self.beta1, 0.999), amsgrad=self.amsgrad, eps=self.eps)
        elif self.optimizer == "RMSProp":
            opt = torch.optim.RMSprop(self.model.parameters(), lr=self.lr, weight_decay=self.weight_decay)
        elif self.optimizer == "SGD":
            opt = torch.optim.SGD(self.model.parameters(), lr=self.lr, momentum=0.9)
        else:
            raise NotImplementedError(f"Optimizer {self.optimizer} not understood.")
        return {"optimizer": opt}

    def optimizer_step(self, *args, **kwargs):
        """models/mcedm.py:163-168, models/ddim.py:228-233: Lightning's step, then EmaModel.update -- which the fused
        optimiser's kernel has already done."""
        super().optimizer_step(*args, **kwargs)
        if self.ema_model is not None and getattr(self, "_fused_opt", None) is None:
            self.ema_model.update(self.model)

    def configure_gradient_clipping(self, optimizer, *args, **kwargs):
        """Lightning calls this between backward and the optimiser's update (configs/trainer/trainer_ddim.yaml:8-9:
        gradient_clip_val 1.0, norm).  With the fused optimiser the clip is not a pass of its own: the value is handed to the
        optimiser, whose kernel scales the gradient by min(1, max_norm / (|g| + 1e-6)) like clip_grad_norm_.  Accepts the hook's
        signatures of pytorch_lightning 1.x (optimizer, optimizer_idx, gradient_clip_val, gradient_clip_algorithm) and 2.x."""
        val, algo = kwargs.get("gradient_clip_val"), kwargs.get("gradient_clip_algorithm")
        pos = list(args)
        if len(pos) == 3:
            pos = pos[1:]                                   # 1.x: optimizer_idx first
        if pos and val is None:
            val = pos[0]
        if len(pos) > 1 and algo is None:
            algo = pos[1]
        algo = getattr(algo, "value", algo)                 # GradClipAlgorithmType enum -> "norm" / "value"
        raw = getattr(optimizer, "_optimizer", optimizer)   # LightningOptimizer wrapper
        fused = getattr(self, "_fused_opt", None)
        if fused is not None and raw is fused and algo in (None, "norm"):
            fused.max_norm = float(val) if val is not None and val > 0 else None
            return
        self.clip_gradients(optimizer, gradient_clip_val=val, gradient_clip_algorithm=algo)

    # ---- data transforms (host-side elementwise, models/mcedm.py:170-197, models/ddim.py:235-262) --------------------
    def data_transform(self, h, u):
        x = torch.cat([self.normalizer_input(h), self.normalizer_target(u)], dim=-1)
        if self.uniform_dequantization:
            x = x / 256.0 * 255.0 + torch.rand_like(x) / 256.0
        if self.gaussian_dequantization:
            x = x + torch.randn_like(x) * 0.01
        return 2 * x - 1.0 if self.rescaled else x

    def inverse_data_transform(self, h, u):
        if self.rescaled:
            h, u = (h + 1.0) / 2.0, (u + 1.0) / 2.0
        if self.normalization == "min_max":
            h, u = torch.clamp(h, 0.0, 1.0), torch.clamp(u, 0.0, 1.0)
        return self.normalizer_input(h, inverse=True), self.normalizer_target(u, inverse=True)

    # ---- HIP path -----------------------------------------------------------------------------------------------------
    def _net(self, model):
        if isinstance(model, EmaModel):
            return model.ma_model
        if isinstance(model, nn.parallel.DistributedDataParallel):
            return model.module
        return model

    def _grad_views(self, params):
        """Views, one per parameter, of the module's flat fp32 gradient buffer (what _TrainLoss.backward scales and returns)."""
        n = sum(p.numel() for p in params)
        if self._grad_buf is None or self._grad_buf.numel() != n or self._grad_buf.device != params[0].device:
            self._grad_buf = torch.empty(n, dtype=torch.float32, device=params[0].device)
        views, off = [], 0
        for p in params:
            views.append(self._grad_buf[off:off + p.numel()].view_as(p))
            off += p.numel()
        return views

    def _cfg_blend(self, xt, sigma, F, Fu, w):
        """Classifier-free blend of the conditioned / unconditioned network outputs and the EDM denoiser of the blend
        (models/mcedm.py:453-458, models/ddim.py:1755-1760)."""
        F = (w + 1) * F - w * Fu
        s = sigma.reshape(-1, 1, 1, 1)
        D = self.sigma_data ** 2 / (s ** 2 + self.sigma_data ** 2) * xt + \
            s * self.sigma_data / (s ** 2 + self.sigma_data ** 2).sqrt() * F
        return D, F

    @staticmethod
    def _churns(sd):
        """Whether any step of the EDM schedule ``sd`` has gamma > 0, i.e. draws churn noise (models/mcedm.py:605-608)."""
        N, t = sd.timesteps, _lib.edm_t_steps(sd)
        return any((min(sd.S_churn / N, math.sqrt(2) - 1) if sd.S_min <= t[i] <= sd.S_max else 0) > 0 for i in range(N))

    def _noise_mode(self):
        """``self.noise_source`` checked ('device', also when a module has no such attribute, or 'torch'): where a sampler's
        per-step noise comes from -- generated inside its kernels from a seed, or drawn by torch into tensors."""
        src = getattr(self, "noise_source", "device")
        if src not in ("device", "torch"):
            raise RuntimeError(f"noise_source must be 'device' or 'torch', not {src!r}")
        return src

    @staticmethod
    def _draw_seed():
        """The key of one call's device-side draws, from torch's CPU generator (no device sync): seed_everything pins a run."""
        return int(torch.randint(0, 2 ** 62, (1,)).item())

    @staticmethod
    def _seed_tensor(seed, device):
        return None if seed is None else torch.tensor([seed], dtype=torch.int64, device=device)

    def _replay(self, key, build, eager, *args, **kw):
        """One sampling call: ``eager(*args, **kw)`` with ``MCEDM_HIP_GRAPH=0``, otherwise replayed from one HIP graph
        (one of lib's Graphed* wrappers, built by ``build()`` on first use).  At most two graphs are kept per module
        (the evaluation loops repeat one call; a ragged last batch is the second), they borrow the module's sampler workspace,
        a failed capture falls back to the eager call, and a replay's static output (a tensor, or a tuple of them) is cloned."""
        if os.environ.get("MCEDM_HIP_GRAPH", "1") == "0":
            return eager(*args, **kw)
        fn = _lib.graphed_or_eager(self._graphs, key, build, eager)
        out = fn(*args, **kw)
        if fn is eager:
            return out
        return tuple(o.clone() for o in out) if isinstance(out, tuple) else out.clone()

    # ---- evaluation bookkeeping both reference loops share (models/ddim.py:235-262, 652-698) ---------------------------
    def _joint_pde_loss(self, x_denoised, x_gt_unnorm=None, noise_level=None, clamp_loss=True, do_rearrange=True, reduce=True):
        """Residual of the joint (h, u) state (models/mcedm.py:460-498, models/ddim.py:535-565)."""
        if do_rearrange:
            x_denoised = x_denoised.permute(0, 2, 3, 1)
        h = x_denoised[..., :self.h_ch].to(torch.float32)
        u = x_denoised[..., self.h_ch:self.h_ch + self.u_ch].to(torch.float32)
        x_un = torch.cat(self.inverse_data_transform(h, u), dim=-1)
        err = self.pde_loss(x_un, x_un if x_gt_unnorm is None else x_gt_unnorm, self.normalizer_input, self.normalizer_target,
                            return_d=False, calc_prob=False, clamp_loss=clamp_loss)
        if noise_level is not None:
            err = err / (noise_level.reshape(-1, 1, 1, 1) + 1.0)
        return err.sum() if reduce else err

    @staticmethod
    def scale_each_min_max(state, return_min_max=False):
        """Per (sample, channel) min-max scaling of a 'b h w c' field to [0, 1] (models/ddim.py:689-698)."""
        b, hh, ww, c = state.shape
        flat = state.permute(0, 3, 1, 2).reshape(b, c, hh * ww)
        lo, hi = flat.min(dim=2, keepdim=True)[0], flat.max(dim=2, keepdim=True)[0]
        scaled = ((flat - lo) / (hi - lo)).reshape(b, c, hh, ww).permute(0, 2, 3, 1)
        return (scaled, lo, hi) if return_min_max else scaled

    @staticmethod
    def scale_back_min_max(state_scaled, state_min, state_max):
        b, hh, ww, c = state_scaled.shape
        flat = state_scaled.permute(0, 3, 1, 2).reshape(b, c, hh * ww) * (state_max - state_min) + state_min
        return flat.reshape(b, c, hh, ww).permute(0, 2, 3, 1)

    def recover_correct_scale(self, gt, xs_scaled_mean):
        _, lo, hi = self.scale_each_min_max(gt, return_min_max=True)
        return self.scale_back_min_max(xs_scaled_mean, lo, hi)

    def get_best_by_pde_error(self, gt, xs_scaled, n_samples, use_gt=True):
        """models/ddim.py:652-674: per input the sample (re-scaled to the ground truth's range) with the smallest mean PDE
        residual; returns (indices [b, 1], the selected scaled samples [b, h, w, c])."""
        gt_rep = gt.repeat(n_samples, 1, 1, 1)
        _, lo, hi = self.scale_each_min_max(gt_rep, return_min_max=True)
        xs_gt = self.scale_back_min_max(xs_scaled, lo, hi)
        err = self.pde_loss(xs_gt, gt_rep if use_gt else xs_gt, self.normalizer_input, self.normalizer_target)
        nb = err.shape[0] // n_samples
        err = err.reshape(n_samples, nb, -1).permute(1, 0, 2).mean(dim=2)                 # '(n b) ... -> b n (...)'
        indices = err.min(dim=1, keepdim=True)[1]
        per_b = xs_scaled.reshape(n_samples, nb, *xs_scaled.shape[1:]).transpose(0, 1)    # b n h w c
        return indices, per_b[torch.arange(nb, device=indices.device), indices[:, 0]]

    def _log(self, name, value):
        self.log(name, value, prog_bar=True, on_epoch=True, on_step=False, sync_dist=True)
