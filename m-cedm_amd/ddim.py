"""Drop-ins for the reference's ``models/ddim.py``.  What they share with each other and with ``PlMcedm`` lives in
``m-cedm_amd/pl_base.py`` (``_PlBase``); this file adds ``_SingleTask`` (conditioning input and evaluation loops of the two
single-task models) and the mixin ``_DdpmSchedule`` (the DDPM schedule as EDM sigmas), like the reference's hierarchy
PlDdim -> PlCondDdim -> PlCondEdm.

``PlDdim``: the joint DDPM baseline sampled with the EDM Heun sampler and
RePaint-style resampling -- ``sample_edm`` (models/ddim.py:959-1051), ``get_denoised`` (:915-947), ``round_sigma``
(:949-957), ``compute_alpha`` (:700-704) on the DDPM U-Net of ``m-cedm_amd/ddim_blocks.py``; the loop runs in
``mcedm_repaint_sample`` (csrc/ddpm.hip).

``PlCondEdm`` for ``models/ddim.py:1608-1773`` (single-task conditional EDM: the
conditioning field h is given, the state u is generated) -- SURVEY.md section 8(f2).

It runs on the same HIP path as ``PlMcedm``: the same ``DhariwalUNet`` (``in_channels`` 1 + ``cond_channels`` 1 ->
``out_ch`` 1 in ``configs/model/adm_edm_cond_h_res32.yaml``), the same EDM preconditioning, and the UNMASKED variants of
the loss and of the Heun sampler (``mask = NULL`` in the C ABI).  Constructor, attributes, state_dict keys (incl. the
DDPM-schedule buffers ``betas`` / ``logvar`` that ``PlDdim.__init__`` registers, models/ddim.py:22-30) and method
signatures follow the reference (incl. PDE guidance, ``dx_cond``, the ``node_type`` channel and the ``cond_p`` drop); DDIM
sampling of ``PlCondEdm`` raises as in the reference (models/ddim.py:1739-1740), and so does ``self_cond`` for it (its sampler
would feed ``denoised`` back).  With a ``name`` that does not start with ``adm`` (configs/model/edm_cond_h_res32.yaml: ``name:
edm_cond_h``, ``cat_cond: True``, ``self_cond: False``) the network is the DDPM U-Net ``Model`` with the conditioning concatenated
to its input, for EVALUATION: ``model_precond``, ``get_denoised``, ``sample_edm`` (with ``guide_dx``), ``validation_step`` and
``test_step`` run on it (mcedm_ddpm_edm_denoise, mcedm_ddpm_edm_heun_sample[_rng]).  ``Model`` has no backward here: with gradients
enabled ``training_step`` and ``forward`` raise; under ``torch.no_grad()`` they run with one noise level per sample
(mcedm_ddpm_edm_denoise_t) and return the reference's ``(output, x0_t)`` and loss value.  ``dx_cond`` raises.

``PlCondDdim`` (bottom of this file) for ``models/ddim.py:1053-1605``: the single-task conditional DDPM on the ADM U-Net with
self-conditioning (which it runs) -- epsilon-prediction ``training_step``, the VP-preconditioned ``sample_edm`` and the DDIM
``sample`` loop in the HIP library.
"""
from __future__ import annotations

import os

import numpy as np
import torch

from . import lib as _lib
from .adm_blocks import DhariwalUNet, EmaModel
from .mcedm import _edm_train_loss
from .pl_base import DotDict, _PlBase, _TrainLoss, _nchw, _opt, correlation, l1, masked_l1


class _SingleTask(_PlBase):
    """What the single-task models (h given, u generated) share -- in the reference PlCondEdm inherits it from PlCondDdim
    (models/ddim.py:1053-1386): the conditioning input, the u-only inverse transform, the PDE residual of (h, u), the
    evaluation loops around ``sample_edm`` and the unroll metrics (``print_unroll_metrics``, ``get_x_unnorm``)."""

    def _adm_only(self, what):
        """With gradients enabled the DDPM U-Net refuses what training calls; under torch.no_grad() it runs (the forward only)."""
        if self._on_ddpm_unet and torch.is_grad_enabled():
            raise NotImplementedError(f"{what} is not built on the DDPM U-Net (models/ddim.py:43-46, Model): it has no backward "
                                      "here; only the ADM U-Net (hparams.name = 'adm*') trains.  Under torch.no_grad() it runs: "
                                      "the noising pass and the loss value, without gradients")

    def _edm_schedule(self, sparams, c_noise_of):
        """The schedule of sample_edm in the reference's own expressions on the host (models/ddim.py:1543-1553, 1566-1567), rounded by
        the module's round_sigma: (N, t_steps fp64 [N + 1], t_hat [N], c_noise [2 N]) with c_noise_of(sigma) the network's label at
        t_hat and at t_next (0 behind the last step, which has no second evaluation)."""
        smin = max(float(sparams.sigma_min), self.sigma_min)
        smax = min(float(sparams.sigma_max), self.sigma_max)
        N, rho = int(sparams.timesteps), float(sparams.rho)
        idx = torch.arange(N, dtype=torch.float64)
        t_steps = (smax ** (1 / rho) + idx / (N - 1) * (smin ** (1 / rho) - smax ** (1 / rho))) ** rho
        t_steps = torch.cat([self.round_sigma(t_steps), torch.zeros_like(t_steps[:1])])
        S_min, S_max = float(sparams.S_min), float(sparams.S_max)
        t_hat, c_noise = [], []
        for i in range(N):
            t_cur = t_steps[i]
            gamma = min(float(sparams.S_churn) / N, np.sqrt(2) - 1) if S_min <= t_cur <= S_max else 0
            th = self.round_sigma(t_cur + gamma * t_cur)
            t_hat.append(float(th))
            c_noise += [c_noise_of(th), c_noise_of(t_steps[i + 1]) if i < N - 1 else 0.0]
        return N, t_steps, t_hat, c_noise

    def inverse_data_transform_u(self, u):
        if self.rescaled:
            u = (u + 1.0) / 2.0
        if self.normalization == "min_max":
            u = torch.clamp(u, 0.0, 1.0)
        return self.normalizer_target(u, inverse=True)

    def get_cond_in(self, h, u, dx, dt):
        """models/ddim.py:1081-1116: h alone, h + the initial condition of u, h + the (t, x) grids, or all of them, by the
        network's conditioning width; node_type appends a channel that is 1 on the boundary of the (t, x) grid and 0 inside."""
        cc = self.model.cond_channels - 1 if self.node_type else self.model.cond_channels
        u_ic = u[:, 0:1].repeat(1, u.shape[1], 1, 1) if u is not None else None
        if cc == self.h_ch:
            cond_in = h
        elif cc == self.h_ch + self.u_ch:
            cond_in = torch.cat([h, u_ic], dim=-1)
        elif cc == self.h_ch + 2:
            cond_in = torch.cat([h, dt, dx], dim=-1)
        elif cc == self.h_ch + self.u_ch + 2:
            cond_in = torch.cat([h, u_ic, dt, dx], dim=-1)
        else:
            raise RuntimeError(f"Number of conditional channels {cc} does not match the known state channels {self.h_ch}")
        if self.node_type:
            b, hc, wc, _ = h.shape
            node = torch.zeros((b, hc, wc, 1), dtype=h.dtype, device=h.device)
            node[:, 0] = 1
            node[:, -1] = 1
            node[:, :, 0] = 1
            node[:, :, -1] = 1
            cond_in = torch.cat([cond_in, node], dim=-1)
        return cond_in

    # ---- the PDE-residual gradient of (h, u): dx_cond's network input and guide_dx's correction, shared by both models ----
    def get_dx_pde(self, cond, x_denoised, calc_prob=False):
        """models/ddim.py:1424-1450: gradient of the PDE residual of (h from cond, u = x_denoised), un-normalised, w.r.t. that
        state; mean (calc_prob) or sum over the two field gradients."""
        h = cond[:, :self.h_ch].to(torch.float32).permute(0, 2, 3, 1)
        u = x_denoised.to(torch.float32).permute(0, 2, 3, 1)
        h_un = self.normalizer_input((h + 1.0) / 2.0 if self.rescaled else h, inverse=True)
        u_un = self.inverse_data_transform_u(u)
        x_un = torch.cat([h_un, u_un], dim=-1).contiguous()
        d = self.pde_loss(x_un, x_un, self.normalizer_input, self.normalizer_target, True, calc_prob).permute(0, 3, 1, 2)
        return torch.mean(d, dim=1, keepdim=True) if calc_prob else torch.sum(d, dim=1)

    def get_dx_input(self, cond, x_denoised):
        """models/ddim.py:601-639 with dx_norm == 'prob' (see the modules' __init__): the log-probability residual gradient itself.  The
        reference's NaN test never fires: both residual classes zero the NaNs of the gradient they return."""
        if not self.dx_cond:
            return None
        return self.get_dx_pde(cond, x_denoised, calc_prob=True).contiguous()

    def get_dx_log_prob(self, cond, x_denoised, guide_dx):
        """models/ddim.py:641-650 (the residual classes already zero the NaNs of the gradient)."""
        if not guide_dx:
            return torch.zeros_like(x_denoised)
        return self.get_dx_pde(cond, x_denoised, calc_prob=True)

    # ---- evaluation loops (models/ddim.py:1154-1319): sampling on the device, metric bookkeeping on the host ----------
    def get_pde_loss(self, cond, x_denoised, x_gt_unnorm=None, noise_level=None, clamp_loss=True, do_rearrange=True,
                     reduce=True):
        """models/ddim.py:1388-1422: residual of (h = the first h_ch conditioning channels, u = x_denoised)."""
        h, u = cond[..., :self.h_ch].to(torch.float32), x_denoised.to(torch.float32)
        if do_rearrange:
            h, u = h.permute(0, 2, 3, 1), u.permute(0, 2, 3, 1)
        x_un = torch.cat(self.inverse_data_transform(h, u), dim=-1)
        err = self.pde_loss(x_un, x_un if x_gt_unnorm is None else x_gt_unnorm, self.normalizer_input, self.normalizer_target,
                            return_d=False, calc_prob=False, clamp_loss=clamp_loss)
        if err.dim() > 3:
            err = err.sum(dim=-1)
        if noise_level is not None:
            err = err / (noise_level.reshape(-1, 1, 1, 1) + 1.0)
        return err.sum() if reduce else err

    def get_x_unnorm(self, cond, x_denoised, do_rearrange=True):
        """models/ddim.py:1378-1386: the un-normalised (h, u) state of a conditioning field and a denoised one."""
        h, u = cond, x_denoised
        if do_rearrange:
            h, u = h.permute(0, 2, 3, 1), u.permute(0, 2, 3, 1)
        return torch.cat(self.inverse_data_transform(h, u), dim=-1)

    def print_unroll_metrics(self, xs, h_unnorm, u_unnorm, state_gt, n_samples):
        """models/ddim.py:1321-1376: run the solver forward from the first row of every recovered state '(n b) t h w c' (its last
        sampler step) and of the truth, and compare the runs.  The n samples go through ONE unroll_loss call (one launch); their
        error sums are then accumulated sample by sample in the reference's order.  Like every PDE entry here the unroll computes
        in fp32 whatever the dtype of xs.  Switches self.pde_loss to the simulator loss, as the reference does."""
        self.pde_loss = self.pde_loss_simulator
        h_ch, u_ch = h_unnorm.shape[-1], u_unnorm.shape[-1]
        n, nb = n_samples, xs.shape[0] // n_samples
        cond = state_gt[..., 0:h_ch]
        pred_unnorm = self.get_x_unnorm(cond.repeat(n, 1, 1, 1), xs[:, -1], do_rearrange=False)
        err, unroll_res = self.pde_loss.unroll_loss(pred_unnorm, pred_unnorm, self.normalizer_input, self.normalizer_target,
                                                    return_unroll=True)
        err = err.reshape(n, nb, *err.shape[1:])
        err_h, err_u = 0.0, 0.0
        for i in range(n):
            err_h += torch.sum(err[i][..., 0:h_ch])
            err_u += torch.sum(err[i][..., h_ch:u_ch + h_ch])
        err_h /= n
        err_u /= n
        x_gt1 = torch.cat([h_unnorm, u_unnorm], dim=-1)
        err_gt, unroll_res_gt = self.pde_loss.unroll_loss(x_gt1, x_gt1, self.normalizer_input, self.normalizer_target,
                                                          return_unroll=True)
        err_gt_h, err_gt_u = torch.sum(err_gt[..., 0:h_ch]), torch.sum(err_gt[..., h_ch:u_ch + h_ch])
        self._log("test_pde_unroll_error", err_u)
        print(f"Tests Unroll error h is {err_h}")
        print(f"Tests Unroll error u is {err_u}")
        self._log("test_pde_unroll_error_gt", err_gt_u)
        print(f"Tests Unroll error gt h is {err_gt_h}")
        print(f"Tests Unroll error gt u is {err_gt_u}")
        gt_rep = unroll_res_gt.repeat(n, 1, 1, 1)
        self._log("test_pde_unrolled_mae_h", l1(unroll_res[..., 0:h_ch], gt_rep[..., 0:h_ch]))
        self._log("test_pde_unrolled_mae_u", l1(unroll_res[..., h_ch:u_ch + h_ch], gt_rep[..., h_ch:u_ch + h_ch]))
        unroll_res = unroll_res.reshape(n, nb, *unroll_res.shape[1:]).permute(1, 2, 3, 0, 4).unsqueeze(1)   # 'b 1 h w n c'
        return unroll_res, unroll_res_gt

    def validation_step(self, val_batch, batch_idx):
        if (self.current_epoch + 1) % 100 != 0 and self.current_epoch != 0:
            return {"epoch": self.current_epoch}
        h_unnorm, dx, dt, u_unnorm = val_batch
        self.h_ch, self.u_ch = h_ch, u_ch = h_unnorm.shape[-1], u_unnorm.shape[-1]
        state_gt = self.data_transform(h_unnorm, u_unnorm)
        h, u = state_gt[..., :h_ch], state_gt[..., h_ch:h_ch + u_ch]
        u_noise = torch.randn_like(u)
        sp = self.sparams
        cond_in = self.get_cond_in(h, u, dx, dt)
        if sp.type == "edm":                                                 # models/ddim.py:1169-1172
            xs = self.sample_edm(cond_in, u_noise, sp, return_last=True, guide_dx=sp.guide_dx)
        else:
            xs, _ = self.sample(cond_in, u_noise, sp, return_last=True, guide_dx=sp.guide_dx)
        last = xs[:, -1]
        loss_u = l1(last[..., :u_ch], u)
        loss_u_un = l1(self.inverse_data_transform_u(last[..., :u_ch]), u_unnorm)
        gt_scaled, xs_scaled = self.scale_each_min_max(state_gt), self.scale_each_min_max(last)
        loss_u_scaled = l1(xs_scaled, gt_scaled[..., h_ch:h_ch + u_ch])
        self._log("val_mae_u", loss_u)
        self._log("val_mae_u_un", loss_u_un)
        self._log("val_mae_u_scaled", loss_u_scaled)
        self._log("val_corr_u", correlation(last, u).mean())
        self._log("val_pde_loss", self.get_pde_loss(h, last, clamp_loss=False, do_rearrange=False) / len(h_unnorm))
        traj, gt = (xs_scaled, gt_scaled[..., h_ch:h_ch + u_ch]) if sp.plot_scaled else (last, u)
        return {"epoch": self.current_epoch, "loss": loss_u, "loss_u_un": loss_u_un, "val_loss_u_scaled": loss_u_scaled,
                "traj": traj.unsqueeze(1), "gt": gt}

    def test_step(self, test_batch, test_idx):
        h_unnorm, dx, dt, u_unnorm = test_batch
        self.h_ch, self.u_ch = h_ch, u_ch = h_unnorm.shape[-1], u_unnorm.shape[-1]
        state_gt = self.data_transform(h_unnorm, u_unnorm)
        h, u = state_gt[..., :h_ch], state_gt[..., h_ch:h_ch + u_ch]
        sp = self.test_sparams
        n, nb = sp.n_samples, len(h_unnorm)
        cond_rep = self.get_cond_in(h, u, dx, dt).repeat(n, 1, 1, 1)
        u_noise = torch.randn_like(u.repeat(n, 1, 1, 1))
        if sp.type == "edm":                                                 # models/ddim.py:1239-1242
            xs = self.sample_edm(cond_rep, u_noise, sp, return_last=sp.return_last, guide_dx=sp.guide_dx)
        else:
            xs, _ = self.sample(cond_rep, u_noise, sp, return_last=sp.return_last, guide_dx=sp.guide_dx)
        xs_mean = xs.reshape(n, nb, *xs.shape[1:]).mean(dim=0)               # '(n b) t h w c -> n b t h w c', mean over n
        u_last = xs_mean[:, -1, :, :, :u_ch]
        loss_u = l1(u_last, u)
        loss_u_un = l1(self.inverse_data_transform_u(u_last), u_unnorm)
        gt_scaled, xs_scaled = self.scale_each_min_max(state_gt), self.scale_each_min_max(xs[:, -1])
        if sp.select_by_pde:                                                 # best sample by PDE error instead of the mean
            print("Use the best sample determined by PDE error")
            h_rep_scaled = self.scale_each_min_max(h.repeat(n, 1, 1, 1).unsqueeze(-1))
            indices, best = self.get_best_by_pde_error(torch.cat([h_unnorm, u_unnorm], dim=-1),
                                                       torch.cat([h_rep_scaled, xs_scaled], dim=-1), n, sp.use_gt_pde_select)
            xs_scaled_mean = best[..., -1:]
            per_b = xs.reshape(n, nb, *xs.shape[1:]).transpose(0, 1)
            xs_mean = per_b[torch.arange(nb, device=indices.device), indices[:, 0]]
        else:
            xs_scaled_mean = xs_scaled.reshape(n, nb, *xs_scaled.shape[1:]).mean(dim=0)
        loss_u_scaled = l1(xs_scaled_mean, gt_scaled[..., h_ch:h_ch + u_ch])
        self._log("test_corr_u", correlation(xs_mean[:, -1], u).mean())
        print(f"\nLoss u {loss_u}, loss u un {loss_u_un}\nLoss u scaled {loss_u_scaled}")
        self._log("test_mae_u", loss_u)
        self._log("test_mae_u_un", loss_u_un)
        self._log("test_mae_u_scaled", loss_u_scaled)
        pde = self.get_pde_loss(state_gt.repeat(n, 1, 1, 1)[..., :h_ch], xs[:, -1], clamp_loss=False, do_rearrange=False) / n / nb
        self._log("test_pde_loss", pde)
        pde_gt = self.get_pde_loss(h, u, clamp_loss=False, do_rearrange=False) / nb
        self._log("test_pde_loss_gt", pde_gt)
        print(f"Pde loss is {pde}\nPde loss gt is {pde_gt}")
        shown = xs_scaled if sp.plot_scaled else xs[:, -1]
        traj = shown.reshape(n, nb, *shown.shape[1:]).permute(1, 2, 3, 0, 4).unsqueeze(1)      # '(n b) h w c -> b 1 h w n c'
        return {"loss": loss_u, "loss_u_un": loss_u_un, "test_mae_u_scaled": loss_u_scaled, "traj": traj,
                "gt": gt_scaled[..., h_ch:h_ch + u_ch] if sp.plot_scaled else u}


def _table_key(t):
    """A host schedule table as part of a graph key: its values are baked into the captured kernel arguments."""
    return hash(t.detach().to("cpu", torch.float32).contiguous().numpy().tobytes())


class _DdpmSchedule:
    """The DDPM noise schedule as EDM sigmas (models/ddim.py:122-137, 949-957), host side: the reference's own expressions on
    CPU tensors.  Mixed into the modules that sample a DDPM network with the EDM sampler (PlDdim, PlCondDdim)."""

    def set_test_sampler_params(self, params):
        self.test_sparams = params
        if params.type == "edm":                                   # models/ddim.py:125-129
            self.edm_steps = self.get_edm_steps()
            self.sigma_min = float(self.edm_steps[self.num_timesteps - 1])
            self.sigma_max = float(self.edm_steps[0])

    def _noise_tables(self, device):
        """sqrt(a) and sqrt(1 - a), a = (1 - betas).cumprod(0), on the module's device (models/ddim.py:195-197)."""
        if getattr(self, "_tables", None) is None or self._tables[0].device != torch.device(device):
            a = (1 - self.betas.to(device)).cumprod(dim=0)
            self._tables = (a.sqrt().contiguous(), (1.0 - a).sqrt().contiguous())
        return self._tables

    def _ddpm_eps_forward(self, x, t, noise, cond):
        """forward(x, t, noise, cond) of the epsilon-prediction modules (models/ddim.py:195-226) on the DDPM U-Net, without
        gradients: (output, x0_t) at one timestep per sample (mcedm_ddpm_forward_t).  torch's generator is consumed as the
        reference consumes it: the cond_p draw (:210), then -- on a self-conditioning network -- the draw of the pre-pass (:214),
        whose estimate mcedm_eps_self_cond writes.  The conditioning map is computed once and serves both passes."""
        net = self.model
        with torch.no_grad():
            x = x.to(torch.float32).contiguous()
            noise = noise.to(torch.float32).contiguous()
            t = torch.as_tensor(t).to(device=x.device, dtype=torch.int64).reshape(-1).contiguous()
            sa, sb = self._noise_tables(x.device)
            x_noise, labels = _lib.eps_noise_inputs(x, noise, t, sa, sb)
            if torch.rand(1) >= self.cond_p:
                cond = None                                    # the conditioning switched off for this batch
            pk = net.packed_weights()
            cmap = None
            if cond is not None:
                if net.cond_enc is None:
                    raise NotImplementedError("cond given to a network built without the cond_enc head")
                cmap = net.plan.cond_map(pk, cond.to(torch.float32).contiguous())

            def x0_of(F):                                      # (x_noise - F sqrt(1 - a)) / sqrt(a), :217 and :224
                out = torch.empty_like(F)
                return _lib.eps_self_cond(out, None, 0, F.shape[1], x_noise=x_noise, F0=F, t=t, sqrt_ab=sa, sqrt_1mab=sb)
            x_sc = None
            if net.self_condition and torch.rand(1) < 0.5:
                x_sc = x0_of(net.plan.forward_t(pk, x_noise, labels, cond_map=cmap, ws=net._ws))
            output = net.plan.forward_t(pk, x_noise, labels, x_self_cond=x_sc, cond_map=cmap, ws=net._ws)
            return output, x0_of(output)

    def _ddpm_eps_loss(self, output, noise):
        """NoiseEstimationLoss (models/losses.py:39-59) of a forward on the DDPM U-Net, the value alone (mcedm_eps_loss)."""
        with torch.no_grad():
            loss = _lib.eps_loss(output, noise.to(torch.float32).contiguous(), want_grad=False)[0].reshape(())
        self.log("train_loss", loss, prog_bar=True, on_epoch=True, on_step=False, sync_dist=True)
        return loss

    def get_edm_steps(self):
        """models/ddim.py:131-137, evaluated on the CPU like the schedule buffers themselves."""
        b = self.betas.detach().cpu()
        alphas_bar = (1.0 - b).cumprod(dim=0)
        return ((1 - alphas_bar) / alphas_bar).sqrt().flip(dims=(0,))

    def _alphas_ext(self):
        b = self.betas.detach().cpu()
        return (1 - torch.cat([torch.zeros(1), b], dim=0)).cumprod(dim=0)

    def round_sigma(self, sigma, return_index=False):
        """models/ddim.py:949-957 (host tensors: the schedule is scalar work)."""
        if self.edm_steps is None:
            raise RuntimeError("call set_test_sampler_params(params) with params.type == 'edm' first (models/ddim.py:122-129)")
        sigma = torch.as_tensor(sigma)
        s32 = sigma.detach().cpu().to(torch.float32)
        index = torch.cdist(s32.reshape(1, -1, 1), self.edm_steps.reshape(1, -1, 1)).argmin(2)
        result = index if return_index else self.edm_steps[index.flatten()]
        return result.to(device=sigma.device).type_as(sigma).reshape(sigma.shape)


class PlCondEdm(_SingleTask):
    def __init__(self, hparams):
        super().__init__()
        self.save_hyperparameters()
        m, o = hparams.model, hparams.optimization
        if _opt(m, "self_cond", False):
            raise NotImplementedError("hparams.model.self_cond=True is outside the MI355X hot path")
        # models/ddim.py:36-38: a boundary / interior flag per grid point rides along as one more conditioning channel
        self.node_type = bool(_opt(m, "node_type", False))
        if self.node_type:
            m.cond_channels = m.cond_channels + 1
        # dx_cond (models/ddim.py:33-35): the network also sees the PDE-residual gradient at its input state.  For the
        # single-task model only dx_norm == 'prob' can run in the reference -- get_dx_pde (:1424-1450) returns a 3-D tensor
        # with calc_prob=False and get_dx_input (:601-639) fails to unpack it (pinned: tests/golden/dxcond.npz
        # 'dx_norm_l2_raises') -- so the other normalisations raise here as well
        self.dx_cond = bool(_opt(m, "dx_cond", False))
        self.dx_norm, self.dx_detach = _opt(m, "dx_norm", "l2"), _opt(m, "dx_detach", False)
        if self.dx_cond and self.dx_norm != "prob":
            raise NotImplementedError(f"dx_cond with dx_norm={self.dx_norm!r}: PlCondEdm.get_dx_input raises in the reference for "
                                      "every dx_norm other than 'prob' (models/ddim.py:608-611, 1445-1448)")
        self._on_ddpm_unet = not str(hparams.name).startswith("adm")                    # models/ddim.py:43-46
        if self._on_ddpm_unet and self.dx_cond:
            raise NotImplementedError("dx_cond (models/ddim.py:33-35) is not built on the DDPM U-Net")
        # DDPM schedule buffers of PlDdim (kept for checkpoint compatibility; the EDM path never reads them)
        self._register_schedule(hparams)
        self.cond_p = _opt(m, "cond_p", 0.8)
        if self._on_ddpm_unet:
            from .ddim_blocks import Model
        self.model = Model(hparams) if self._on_ddpm_unet else DhariwalUNet(hparams)
        self.ema_model = EmaModel(self.model, beta=m.ema_rate) if m.ema else None
        # models/ddim.py:68-72: the PDE residual term of training_step (mcedm_pde_train_loss)
        self.pde_loss_lambda = _opt(o, "pde_loss_lambda", 0.0)
        self.pde_loss_prop_t = _opt(o, "pde_loss_prop_t", False)
        self.use_gt_pde = _opt(o, "use_gt_pde", False)
        self._init_common(hparams, m.in_channels, m.out_ch, default_sampler=self.get_edm_sampler_params)
        self.P_mean, self.P_std, self.sigma_data = -1.2, 1.2, 1.0
        self.sigma_min, self.sigma_max = 0.002, 80
        self.noise_source = os.environ.get("MCEDM_NOISE_SOURCE", "device")      # the sampler's churn draws, as in PlMcedm
        # a default until the first batch sets the widths (the reference has none: models/ddim.py:1120-1121 are its first
        # assignments); the node_type channel added above is not part of the known state
        self.h_ch, self.u_ch = m.cond_channels - (1 if self.node_type else 0), m.out_ch

    # ---- configuration ----------------------------------------------------------------------------------
    @staticmethod
    def get_edm_sampler_params():
        return DotDict(name="edm", type="edm", timesteps=50, sigma_min=0.002, sigma_max=80, rho=7, S_churn=15.0, S_min=0,
                       S_max="inf", S_noise=1, n_samples=5, n_repeat=2, n_time_h=128, n_time_u=0, return_last=True,
                       select_by_pde=False, use_gt_pde_select=True, guide_dx=False, w=0.0, plot_scaled=False)

    def set_test_sampler_params(self, params):
        if params.type != "edm":
            print("Model with EDM preconditioning supports only EDM sampler ")
            params = self.get_edm_sampler_params()
        self.test_sparams = params

    def configure_optimizers(self):
        if self.optimizer != "Adam":
            raise NotImplementedError(f"Optimizer {self.optimizer} not understood.")
        return {"optimizer": torch.optim.Adam(self.model.parameters(), lr=self.lr, weight_decay=self.weight_decay,
                                              betas=(self.beta1, 0.999), amsgrad=self.amsgrad, eps=self.eps)}

    def get_loss_weight(self, sigma):
        return (sigma ** 2 + self.sigma_data ** 2) / (sigma * self.sigma_data) ** 2

    def round_sigma(self, sigma, return_index=False):
        """models/ddim.py:1765-1768: the EDM schedule is continuous, nothing is rounded."""
        sigma = torch.as_tensor(sigma)
        return 0 if return_index else sigma

    def forward(self, x, sigma, noise, cond=None):
        """models/ddim.py:1668-1694 on the DDPM U-Net without gradients: (output, x0_t) with one noise level per sample."""
        self._adm_only("forward (the noising pass of training)")
        if not self._on_ddpm_unet:
            return super().forward(x, sigma, noise, cond)      # not defined for the ADM U-Net: training_step is the entry
        with torch.no_grad():
            sigma = torch.as_tensor(sigma).to(device=x.device, dtype=torch.float32)
            x_noise = x.to(torch.float32) + noise.to(torch.float32) * sigma.reshape(-1, 1, 1, 1)
            if torch.rand(1) >= self.cond_p:
                cond = None                                    # the conditioning switched off for this batch (:1683-1684)
            output = self.model_precond(x_noise, sigma, cond)  # no self-conditioning on this network: no pre-pass, no draw
        return output, output

    # ---- HIP path -------------------------------------------------------------------------------------------
    def _dx_arg(self, net, dx):
        if dx is None:
            return None
        if not net.dx_cond:
            raise NotImplementedError("dx given to a network built with dx_cond=False (the reference ignores it silently)")
        return dx.to(torch.float32).contiguous()

    def _ddpm_denoise(self, net, xt, sigma, cond, dx, w):
        """get_denoised / model_precond on the DDPM U-Net (mcedm_ddpm_edm_denoise): one noise level, c_noise = sigma.log() / 4 in
        torch's fp32 like the reference (:1661, 1753); the conditioning is concatenated unscaled."""
        if dx is not None:
            raise NotImplementedError("dx_cond is not built on the DDPM U-Net")
        sig = torch.as_tensor(sigma).detach().to("cpu", torch.float32).reshape(-1)
        if sig.numel() != 1 and not bool((sig == sig[0]).all()):
            guided = w is not None and abs(w) >= 0.001
            if torch.is_grad_enabled() or guided or sig.numel() != xt.shape[0]:
                raise NotImplementedError("one noise level for the whole batch (what sample_edm evaluates); a level per sample "
                                          "runs under torch.no_grad(), without guidance (mcedm_ddpm_edm_denoise_t)")
            return net.plan.edm_denoise_t(net.packed_weights(), xt.to(torch.float32).contiguous(),
                                          torch.as_tensor(sigma).detach().to(xt.device, torch.float32).reshape(-1).contiguous(),
                                          cond=None if cond is None else cond.to(torch.float32).contiguous(),
                                          sigma_data=self.sigma_data, ws=net._ws, want_F=True)
        c_noise = float((sig[:1].log() / 4)[0])
        with torch.no_grad():
            return net.plan.edm_denoise(net.packed_weights(), xt.to(torch.float32).contiguous(), float(sig[0]), c_noise,
                                        cond=None if cond is None else cond.to(torch.float32).contiguous(),
                                        w=0.0 if w is None else float(w), sigma_data=self.sigma_data, ws=net._ws, want_F=True)

    def model_precond(self, x_noise, sigma, cond=None, x_self_cond=None, dx=None):
        if x_self_cond is not None:
            raise NotImplementedError("x_self_cond is outside the hot path")
        net = self.model
        if self._on_ddpm_unet:
            return self._ddpm_denoise(net, x_noise, sigma, cond, dx, None)[0]
        with torch.no_grad():
            return net.plan.denoise(net.packed_weights(), x_noise.float().contiguous(),
                                    sigma.to(torch.float32).reshape(-1).contiguous(),
                                    cond=None if cond is None else cond.float().contiguous(), ws=net._ws,
                                    sigma_data=self.sigma_data, dx=self._dx_arg(net, dx))

    def get_denoised(self, model, xt, t, cond=None, x_self_cond=None, dx=None, w=None):
        if x_self_cond is not None:
            raise NotImplementedError("x_self_cond is outside the hot path")
        net = self._net(model)
        if self._on_ddpm_unet:
            return self._ddpm_denoise(net, xt, t, cond, dx, w)
        xt = xt.to(torch.float32).contiguous()
        sigma = torch.as_tensor(t).to(torch.float32).reshape(-1).contiguous().to(xt.device)
        cond = None if cond is None else cond.float().contiguous()
        dx = self._dx_arg(net, dx)
        pk = net.packed_weights()
        with torch.no_grad():
            D, F = net.plan.denoise(pk, xt, sigma, cond=cond, ws=net._ws, sigma_data=self.sigma_data, want_F=True, dx=dx)
            # models/ddim.py:1755-1760: the branch is taken when cond OR dx is given; its second evaluation drops both
            if not (w is None or abs(w) < 0.001 or (cond is None and dx is None)):
                _, Fu = net.plan.denoise(pk, xt, sigma, cond=None, ws=net._ws, sigma_data=self.sigma_data, want_F=True)
                D, F = self._cfg_blend(xt, sigma, F, Fu, w)
        return D, F

    def training_step(self, train_batch, batch_idx):
        self._adm_only("training_step")
        h_unnorm, dx, dt, u_unnorm = train_batch
        self.h_ch, self.u_ch = h_ch, u_ch = h_unnorm.shape[-1], u_unnorm.shape[-1]
        if self.pde_loss_lambda > 0.:
            self._pde_train_check()
        x = self.data_transform(h_unnorm, u_unnorm)
        h, u = x[..., 0:h_ch], x[..., h_ch:h_ch + u_ch]
        cond_in = _nchw(self.get_cond_in(h, u, dx, dt)).float()
        u = _nchw(u).float()
        noise = torch.randn_like(u)
        rnd_normal = torch.randn([u.shape[0], 1, 1, 1]).type_as(u)
        u_noise, sigma = _lib.edm_noise_inputs(u, None, noise, rnd_normal.reshape(-1).contiguous(), self.P_mean, self.P_std)
        dx = None
        if self.dx_cond and torch.rand(1) > 0.1:                 # models/ddim.py:1672-1677: dx off with a small probability
            dx = self.get_dx_input(cond_in[:, 0:self.h_ch], u_noise)     # on the NOISED target; carries no gradient
        if torch.rand(1) >= self.cond_p:                         # models/ddim.py:1683-1684: conditioning off for this batch
            cond_in = None                                       # (the network then reads zeros, adm_blocks.py:328-331)
        # models/ddim.py:1726-1731: pde_loss_lambda * get_pde_loss(h, x0_t, ..., clamp_loss=True) on top of the EDM loss.  h is
        # the normalised data (not cond_in: the cond_p draw does not remove it), read in place as a channel slice of x.  The
        # reference's own call raises (:1729 passes the channel-last h with do_rearrange=True; :1396 scrambles it, :1400 cannot
        # concatenate): this is the residual of (h, x0_t) in one layout, as validation_step / test_step form it
        pde = self._pde_train_args(h_unnorm, u_unnorm, sigma) if self.pde_loss_lambda > 0. else None
        parts = {}

        def pde_term(D, dD, edm):
            """pde_loss of the denoised D, its gradient accumulated into the EDM loss's dD; edm + lambda * pde in fp32."""
            parts["edm"] = edm.reshape(())
            parts["pde"] = _lib.pde_train_loss(pde[0], D, h, gt=pde[1], w=pde[2], dD=dD)[0].reshape(())
            return parts["edm"] + self.pde_loss_lambda * parts["pde"]

        if self._on_ddpm_unet:                                   # under torch.no_grad() (see _adm_only): the loss value alone
            D = self.model_precond(u_noise, sigma, cond_in)
            loss = _lib.edm_loss(D, u.contiguous(), None, sigma, self.sigma_data, want_grad=False)[0].reshape(())
            if pde is not None:
                loss = pde_term(D, None, loss)
        else:
            loss = _edm_train_loss(self, u, u_noise, sigma, cond_in, None, dx, pde_term if pde is not None else None)
        # train_loss is the EDM part: the reference logs it before it adds the PDE term (:1724)
        self.log("train_loss", parts["edm"].detach() if pde is not None else loss, prog_bar=True, on_epoch=True, on_step=False,
                 sync_dist=True)
        if pde is not None:
            self.log("train_pde_loss", parts["pde"], prog_bar=True, on_epoch=True, on_step=False, sync_dist=True)
        return loss

    def _pde_train_check(self):
        """The PDE term is built for what the guided sampler is built for: one gauss-normalised channel per field, no flip."""
        if self.pde_loss is None or not hasattr(self.pde_loss, "guidance_desc"):
            raise RuntimeError("pde_loss_lambda > 0 needs set_pde_loss_function('swe' | 'swe_per' | 'darcy') before training_step")
        if self.pde_loss.flip_xy:
            raise NotImplementedError("pde_loss_lambda > 0 with flip_xy (flip_state, models/pde_loss.py:6-16, 228-229) is not built")
        if self.rescaled:
            raise NotImplementedError("pde_loss_lambda > 0 with data.rescaled (inverse_data_transform, models/ddim.py:251-262) is not built")
        if self.normalization == "min_max":
            raise NotImplementedError("pde_loss_lambda > 0 with min_max normalisation (the clamp of inverse_data_transform, "
                                      "models/ddim.py:251-262) is not built")
        if self.h_ch != 1 or self.u_ch != 1:
            raise NotImplementedError("pde_loss_lambda > 0 with more than one channel per field (models/ddim.py:1390-1400) is not built")

    def _pde_train_args(self, h_unnorm, u_unnorm, sigma):
        """(description, gt, w) of mcedm_pde_train_loss for this batch."""
        gd = self.pde_loss.guidance_desc(self.normalizer_input, self.normalizer_target, h_unnorm.shape[1], h_unnorm.shape[2],
                                         weight=float(self.pde_loss_lambda))
        # use_gt_pde (:1728): the data as the residual's target, without a gradient; otherwise the denoised state itself
        gt = torch.cat([h_unnorm, u_unnorm], dim=-1).to(torch.float32).contiguous() if self.use_gt_pde else None
        # pde_loss_prop_t (:1727, 1413-1416): the (b, t, x) matrix divided by noise_level.reshape(-1, 1, 1, 1) + 1 broadcasts to
        # (b, b, t, x), so every sample's residual meets every noise level: the factor is sum_i 1 / (sigma_i + 1) for all of them
        w = (1.0 / (sigma + 1.0)).sum().expand(sigma.numel()).contiguous() if self.pde_loss_prop_t else None
        return gd, gt, w

    def sample(self, h, u_noise, sparams, return_last=True, guide_dx=False):
        raise NotImplementedError("Only EDM sampler is supported for the model with EDM pre-conditioning")      # models/ddim.py:1739-1740

    def sample_edm(self, h, u_noise, sparams, return_last=True, guide_dx=False):
        """h, u_noise in the reference's 'b h w c' layout; returns [b, t, h, w, c] float64 (models/ddim.py:1532-1601).
        guide_dx=True: after every denoiser call d -= 5 * dx / t_hat with dx the PDE-residual gradient, evaluated on the
        device by the stencils' analytic adjoints (csrc/pde.hip) instead of torch.autograd.
        The per-step churn noise is generated inside the churn kernel from a seed drawn from torch's CPU generator
        (``noise_source = "device"``), or drawn with torch.randn as one [N, B, C, H, W] float64 tensor (``"torch"``)."""
        noise_source = self._noise_mode()
        guidance = dx_input = None
        if guide_dx or self.dx_cond:
            if self.pde_loss is None or not hasattr(self.pde_loss, "guidance_desc"):
                raise NotImplementedError("guide_dx / dx_cond need set_pde_loss_function('swe' | 'swe_per' | 'darcy')")
            if self.rescaled or self.normalization == "min_max" or self.h_ch != 1 or self.u_ch != 1:
                raise NotImplementedError("guide_dx / dx_cond are built for scalar gauss-normalised fields h, u")
            gdesc = self.pde_loss.guidance_desc(self.normalizer_input, self.normalizer_target, h.shape[1], h.shape[2])
            guidance = gdesc if guide_dx else None
            # dx_cond: dx_in = get_dx_input(h, x) on the current noisy state before every denoiser call (:1571, :1584)
            dx_input = gdesc if self.dx_cond else None
        net = self._net(self.ema_model if self.ema_model is not None else self.model)
        if self._on_ddpm_unet:
            return self._ddpm_sample_edm(net, h, u_noise, sparams, return_last, guidance, noise_source)
        h, init = _nchw(h).float(), _nchw(u_noise).float()
        sd = _lib.sampler_desc(sparams, self.sigma_data, self.sigma_min, self.sigma_max)
        N, churn = sd.timesteps, self._churns(sd)
        dev_noise = churn and noise_source == "device"
        step_noise = (torch.randn((N,) + tuple(init.shape), dtype=torch.float64, device=init.device)
                      if churn and not dev_noise else None)
        kw = dict(seed=self._draw_seed()) if dev_noise else {}
        with torch.no_grad():
            packed = net.packed_weights()
            eager = lambda c, m_, i, sn, seed=None: net.plan.sample(      # noqa: E731
                packed, sd, c, None, i, sn, return_last=return_last, ws=self._sample_ws, guidance=guidance, dx_input=dx_input,
                rng_seed=self._seed_tensor(seed, i.device))
            # the call replays from one HIP graph, like PlMcedm.sample_edm (the evaluation loops repeat it); the residual
            # descriptions of guide_dx / dx_cond are host-side structs, so they are part of the key and of the capture
            B, _, H, W = init.shape
            dkey = lambda d: None if d is None else _lib.desc_key(d)      # noqa: E731
            key = (B, H, W, bool(return_last), churn, dev_noise, packed.data_ptr(), init.device.index,
                   _lib.desc_key(sd), dkey(guidance), dkey(dx_input))
            return self._replay(key, lambda: _lib.GraphedSampler(
                net.plan, packed, sd, B, H, W, masked=False, has_cond=True, churn=churn, return_last=return_last,
                ws=self._sample_ws, guidance=guidance, dx_input=dx_input, device_noise=dev_noise), eager, h, None, init,
                step_noise, **kw)


    def _ddpm_sample_edm(self, net, h, u_noise, sparams, return_last, guidance, noise_source):
        """sample_edm on the DDPM U-Net: the schedule in the reference's own expressions on the host (:1543-1553, 1566-1567;
        round_sigma is the identity: _edm_schedule), c_noise = ln(sigma) / 4 in torch's fp32 at t_hat and at t_next; the loop runs in
        mcedm_ddpm_edm_heun_sample[_rng] and replays from one HIP graph."""
        h, init = _nchw(h).float().contiguous(), _nchw(u_noise).float().contiguous()
        N, t_steps, t_hat, c_noise = self._edm_schedule(
            sparams, lambda t: float((t.to(torch.float32).reshape(1).log() / 4)[0]))      # (:1747-1753)
        cond = h if net.cond_channels > 0 else None
        vd = _lib.vp_sampler_desc(N, net.cond_channels if cond is not None else 0, t_steps.tolist(), t_hat, c_noise,
                                  float(sparams.S_noise), float(sparams.w))
        churn = any(th != float(t_steps[i]) for i, th in enumerate(t_hat))     # the steps whose x_hat adds noise (:1567)
        dev_noise = churn and noise_source == "device"
        step_noise = (torch.randn((N,) + tuple(init.shape), dtype=torch.float64, device=init.device)
                      if churn and not dev_noise else None)
        kw = dict(seed=self._draw_seed()) if dev_noise else {}
        with torch.no_grad():
            packed = net.packed_weights()
            eager = lambda c, i, sn, seed=None: net.plan.edm_sample(      # noqa: E731
                packed, vd, c, i, sn, return_last=return_last, ws=self._sample_ws, rng_seed=self._seed_tensor(seed, i.device),
                sigma_data=self.sigma_data, guidance=guidance)
            B = init.shape[0]
            key = ("ddpm_edm", B, bool(return_last), churn, dev_noise, packed.data_ptr(), init.device.index, N, vd.cond_channels,
                   tuple(t_steps.tolist()), tuple(t_hat), tuple(c_noise), float(sparams.S_noise), float(sparams.w),
                   float(self.sigma_data), None if guidance is None else _lib.desc_key(guidance))
            return self._replay(key, lambda: _lib.GraphedDdpmEdmSampler(
                net.plan, packed, vd, B, cond is not None, churn, return_last=return_last, ws=self._sample_ws,
                device_noise=dev_noise, sigma_data=self.sigma_data, guidance=guidance), eager, cond, init, step_noise, **kw)


class PlDdim(_DdpmSchedule, _PlBase):
    """models/ddim.py:16-1051, the part BASELINE config 5 exercises: EDM / RePaint sampling of the joint (h, u) DDPM.
    Constructor, buffers (``betas``, ``logvar``), attributes and the signatures of ``set_test_sampler_params``,
    ``get_edm_steps``, ``compute_alpha``, ``round_sigma``, ``get_denoised`` and ``sample_edm`` follow the reference.
    ``sample_with_repeat`` (the DDIM sampler with RePaint loops, the default ``diff_sampler: ddim_sampler``) runs on the device
    too (round 3).  DDPM training (``Model`` has no backward: with gradients enabled ``training_step`` and ``forward`` raise; under
    ``torch.no_grad()`` they run with one timestep per sample, mcedm_ddpm_forward_t, and return the reference's ``(output, x0_t)``
    and loss value), the h -> u ``sample`` loop and PDE guidance are not built and raise."""

    def __init__(self, hparams):
        super().__init__()
        self.save_hyperparameters()
        m = hparams.model
        for flag in ("dx_cond", "node_type"):
            if _opt(m, flag, False):
                raise NotImplementedError(f"hparams.model.{flag}=True is outside the built path")
        if str(hparams.name).startswith("adm"):
            raise NotImplementedError("PlDdim with the ADM U-Net is not built; use PlMcedm / PlCondEdm for ADM networks")
        from .ddim_blocks import Model
        self._register_schedule(hparams)
        self.cond_p = 0.0
        self.dx_cond = self.node_type = False
        self.model = Model(hparams)
        self.ema_model = EmaModel(self.model, beta=m.ema_rate) if m.ema else None
        self.h_ch = self.u_ch = m.out_ch // 2
        self._init_common(hparams, self.h_ch, self.u_ch)
        self.edm_steps = self.sigma_min = self.sigma_max = None
        self.pde_loss_lambda = _opt(_opt(hparams, "optimization", None), "pde_loss_lambda", 0.0)

    def compute_alpha(self, t):
        """models/ddim.py:700-704."""
        return self._alphas_ext().index_select(0, torch.as_tensor(t).cpu().reshape(-1) + 1).view(-1, 1, 1, 1)

    def get_denoised(self, model, xt, t, cond=None, x_self_cond=None, dx=None, w=None):
        """models/ddim.py:915-947 at one noise level: VP preconditioning around the DDPM network."""
        if cond is not None or x_self_cond is not None or dx is not None:
            raise NotImplementedError("cond / x_self_cond / dx are outside the built path")
        net = self._net(model)
        t = torch.as_tensor(t).reshape(-1)
        if t.numel() != 1:
            raise NotImplementedError("one noise level for the whole batch (what sample_edm evaluates)")
        sigma = t.to(torch.float32)
        c_noise = self.num_timesteps - 1 - self.round_sigma(sigma.reshape(1, 1, 1, 1), return_index=True).to(torch.float32)
        with torch.no_grad():
            return net.plan.denoise(net.packed_weights(), xt.to(torch.float32).contiguous(), float(sigma), float(c_noise),
                                    ws=net._ws, want_F=True)

    # ---- sampling -----------------------------------------------------------------------------------------------
    def sample_edm(self, h, u, sparams, return_last=True, guide_dx=False):
        """models/ddim.py:959-1051.  h, u: 'b h w c' normalised fields; returns [b, t, h, w, c] float64.
        The known region is rows < n_time_h of h and rows < n_time_u of u; every step runs n_repeat Heun updates with the
        known region re-noised to the current level in between (RePaint).

        Noise: the initial ``randn_like(hu)`` is torch's; the per-step and per-loop draws (timesteps * n_repeat tensors in the
        reference, :1004 / :1037) are generated INSIDE the re-noising kernels from a 64-bit seed drawn from torch's generator
        (``self.noise_source = "device"``, the default: no noise tensors exist and the call replays from one HIP graph), or
        drawn with torch.randn into two tensors (``"torch"``: what the golden tests inject into)."""
        if guide_dx:
            raise NotImplementedError("guide_dx=True (PDE guidance) is outside the built path")
        if self.edm_steps is None:
            self.set_test_sampler_params(sparams)
        net = self._net(self.ema_model if self.ema_model is not None else self.model)
        hu = _nchw(torch.cat([h, u], dim=-1)).float()
        rd, keep = _lib.repaint_desc(sparams, self.edm_steps, self._alphas_ext(), self.h_ch, self.u_ch)
        hu_noise = torch.randn_like(hu)
        N, R = rd.timesteps, rd.n_repeat
        packed = net.packed_weights()
        with torch.no_grad():
            if getattr(self, "noise_source", "device") == "torch":
                churn = float(sparams.S_churn) > 0
                step_noise = torch.randn((N,) + tuple(hu.shape), dtype=torch.float64, device=hu.device) if churn else None
                repeat_noise = torch.randn((N, R - 1) + tuple(hu.shape), dtype=torch.float64, device=hu.device) if R > 1 else None
                return net.plan.repaint_sample(packed, rd, hu, hu_noise, step_noise, repeat_noise, return_last=return_last,
                                               ws=self._sample_ws)
            seed = torch.randint(0, 2 ** 62, (1,), dtype=torch.int64)          # CPU generator: torch.manual_seed reproduces
            eager = lambda x, nz, sd: net.plan.repaint_sample(packed, rd, x, nz, return_last=return_last, ws=self._sample_ws,
                                                              rng_seed=sd.to(x.device))
            B = hu.shape[0]
            key = (B, bool(return_last), packed.data_ptr(), hu.device.index, float(self.edm_steps[0]),
                   _lib.desc_key(rd, skip=("edm_steps", "alphas_cumprod_ext")))
            return self._replay(key, lambda: _lib.GraphedRepaint(net.plan, packed, rd, keep, B, return_last, ws=self._sample_ws),
                                eager, hu, hu_noise, seed)

    # ---- evaluation loops (models/ddim.py:294-533): BASELINE config 5 is run through trainer.test -> test_step ------------
    def get_pde_loss(self, cond, x_denoised, x_gt_unnorm=None, noise_level=None, clamp_loss=True, do_rearrange=True,
                     reduce=True):
        """models/ddim.py:535-565: residual of the joint (h, u) state."""
        return self._joint_pde_loss(x_denoised, x_gt_unnorm, noise_level, clamp_loss, do_rearrange, reduce)

    def _sample_eval(self, h, u, sp, return_last):
        """models/ddim.py:309-312, 391-394: the EDM / RePaint sampler for type 'edm', the DDIM RePaint sampler otherwise."""
        if sp.type == "edm":
            return self.sample_edm(h, u, sp, return_last=return_last, guide_dx=sp.guide_dx)
        return self.sample_with_repeat(h, u, sp, return_last=return_last, guide_dx=sp.guide_dx)[0]

    def validation_step(self, val_batch, batch_idx):
        if (self.current_epoch + 1) % 100 != 0 and self.current_epoch != 0:
            return {"epoch": self.current_epoch}
        h_unnorm, dx, dt, u_unnorm = val_batch
        self.h_ch, self.u_ch = h_ch, u_ch = h_unnorm.shape[-1], u_unnorm.shape[-1]
        state_gt = self.data_transform(h_unnorm, u_unnorm)
        h, u = state_gt[..., :h_ch], state_gt[..., h_ch:h_ch + u_ch]
        sp = self.sparams
        # the reference hands NOISE in as the u field here (models/ddim.py:306-309): rows < n_time_u of it count as known
        xs = self._sample_eval(h, torch.randn_like(u), sp, True)
        last = xs[:, -1]
        h_last, u_last = last[..., :h_ch], last[..., h_ch:h_ch + u_ch]
        loss_h, loss_u = l1(h_last, h), l1(u_last, u)
        h_un, u_un = self.inverse_data_transform(h_last, u_last)
        loss_h_un, loss_u_un = l1(h_un, h_unnorm), l1(u_un, u_unnorm)
        gt_scaled, xs_scaled = self.scale_each_min_max(state_gt), self.scale_each_min_max(last)
        loss_h_scaled = l1(xs_scaled[..., :h_ch], gt_scaled[..., :h_ch])
        loss_u_scaled = l1(xs_scaled[..., h_ch:h_ch + u_ch], gt_scaled[..., h_ch:h_ch + u_ch])
        for name, v in (("val_mae_h", loss_h), ("val_mae_u", loss_u), ("val_mae_h_un", loss_h_un), ("val_mae_u_un", loss_u_un),
                        ("val_mae_h_scaled", loss_h_scaled), ("val_mae_u_scaled", loss_u_scaled)):
            self._log(name, v)
        corr = correlation(last, state_gt)
        self._log("val_corr_h", corr[:h_ch].mean())
        self._log("val_corr_u", corr[h_ch:h_ch + u_ch].mean())
        self._log("val_pde_loss", self.get_pde_loss(None, last, clamp_loss=False, do_rearrange=False) / len(h_unnorm))
        traj, gt = (xs_scaled, gt_scaled) if sp.plot_scaled else (last, state_gt)
        return {"epoch": self.current_epoch, "loss_h": loss_h, "loss": loss_u, "loss_h_un": loss_h_un, "loss_u_un": loss_u_un,
                "val_loss_h_scaled": loss_h_scaled, "val_loss_u_scaled": loss_u_scaled, "traj": traj.unsqueeze(1), "gt": gt}

    def test_step(self, test_batch, test_idx):
        h_unnorm, dx, dt, u_unnorm = test_batch
        self.h_ch, self.u_ch = h_ch, u_ch = h_unnorm.shape[-1], u_unnorm.shape[-1]
        hs, us = slice(0, h_ch), slice(h_ch, h_ch + u_ch)
        state_gt = self.data_transform(h_unnorm, u_unnorm)
        h, u = state_gt[..., hs], state_gt[..., us]
        sp = self.test_sparams
        n, nb = sp.n_samples, len(h_unnorm)
        rep = state_gt.repeat(n, 1, 1, 1)
        n_all, n_time_h, n_time_u = h.shape[1], sp.n_time_h, sp.n_time_u
        xs = self._sample_eval(rep[..., hs], rep[..., us], sp, sp.return_last)
        xs_mean = xs.reshape(n, nb, *xs.shape[1:]).mean(dim=0)               # '(n b) t h w c -> n b t h w c', mean over n
        h_last, u_last = xs_mean[:, -1, :, :, hs], xs_mean[:, -1, :, :, us]
        loss_h, loss_u = l1(h_last, h), l1(u_last, u)
        h_un, u_un = self.inverse_data_transform(h_last, u_last)
        loss_h_un, loss_u_un = l1(h_un, h_unnorm), l1(u_un, u_unnorm)
        hu_un, gt_un = torch.cat([h_un, u_un], dim=-1), torch.cat([h_unnorm, u_unnorm], dim=-1)
        unknown = torch.ones_like(hu_un)                                     # 1 = generated entries (:419-424)
        if n_time_h > 0:
            unknown[:, :n_time_h, :, hs] = 0.0
        if n_time_u > 0:
            unknown[:, :n_time_u, :, us] = 0.0
        loss_hu_un = masked_l1(hu_un, gt_un, unknown)
        gt_scaled, xs_scaled = self.scale_each_min_max(state_gt), self.scale_each_min_max(xs[:, -1])
        if sp.select_by_pde:
            print("Use the best sample determined by PDE error")
            indices, xs_scaled_mean = self.get_best_by_pde_error(gt_un, xs_scaled, n, sp.use_gt_pde_select)
            per_b = xs.reshape(n, nb, *xs.shape[1:]).transpose(0, 1)
            xs_mean = per_b[torch.arange(nb, device=indices.device), indices[:, 0]]
        else:
            xs_scaled_mean = xs_scaled.reshape(n, nb, *xs_scaled.shape[1:]).mean(dim=0)
        loss_h_scaled = l1(xs_scaled_mean[..., hs], gt_scaled[..., hs])
        loss_u_scaled = l1(xs_scaled_mean[..., us], gt_scaled[..., us])
        corr = correlation(xs_mean[:, -1], state_gt)
        self._log("test_corr_h", corr[hs].mean())
        self._log("test_corr_u", corr[us].mean())
        for tag, ch, last, ref, k, on in (("h", hs, h_last, h, n_time_h, n_time_h < n_all),
                                          ("u", us, u_last, u, n_time_u, n_all > n_time_u > 0)):
            if on:      # error on the rows handed in (0 by construction) and scaled error on / off them (:460-482)
                self._log(f"test_{tag}_known", l1(last[:, :k], ref[:, :k]))
                self._log(f"test_{tag}_kn_scaled", l1(xs_scaled_mean[:, :k, :, ch], gt_scaled[:, :k, :, ch]))
                self._log(f"test_{tag}_unkn_scaled", l1(xs_scaled_mean[:, k:, :, ch], gt_scaled[:, k:, :, ch]))
        print(f"\nLoss h {loss_h}, loss h un {loss_h_un}\nLoss u {loss_u}, loss u un {loss_u_un}\nLoss hu un {loss_hu_un}\n"
              f"Loss h scaled {loss_h_scaled}, loss u scaled {loss_u_scaled}")
        for name, v in (("test_mae_h", loss_h), ("test_mae_u", loss_u), ("test_mae_h_un", loss_h_un), ("test_mae_u_un", loss_u_un),
                        ("test_mae_hu_un", loss_hu_un), ("test_mae_h_scaled", loss_h_scaled), ("test_mae_u_scaled", loss_u_scaled)):
            self._log(name, v)
        pde = self.get_pde_loss(None, xs[:, -1], clamp_loss=False, do_rearrange=False) / n / nb
        self._log("test_pde_loss", pde)
        pde_gt = self.get_pde_loss(None, state_gt, clamp_loss=False, do_rearrange=False) / nb
        self._log("test_pde_loss_gt", pde_gt)
        print(f"Pde loss is {pde}\nPde loss gt is {pde_gt}")
        if sp.return_last:                 # the last state of every sample: '(n b) h w c -> b 1 h w n c'
            last = xs[:, -1]
            xs_plot = last.reshape(n, nb, *last.shape[1:]).permute(1, 2, 3, 0, 4).unsqueeze(1)
            sc_plot = xs_scaled.reshape(n, nb, *xs_scaled.shape[1:]).permute(1, 2, 3, 0, 4).unsqueeze(1)
        else:                              # every second state of the FIRST sample, time steps in the sample slot (:518-525)
            first = xs[:, ::2].reshape(n, nb, *xs[:, ::2].shape[1:])[0]               # b t h w c
            nt = first.shape[1]
            xs_plot = first.reshape(nb * nt, *first.shape[2:])                          # '(b t) h w c'
            sc = self.scale_each_min_max(xs_plot)
            sc_plot = sc.reshape(nb, nt, *sc.shape[1:]).permute(0, 2, 3, 1, 4).unsqueeze(1)   # 'b 1 h w t c'
        return {"loss_h": loss_h, "loss": loss_u, "loss_h_un": loss_h_un, "loss_u_un": loss_u_un,
                "test_mae_u_scaled": loss_u_scaled, "traj": sc_plot if sp.plot_scaled else xs_plot,
                "gt": gt_scaled if sp.plot_scaled else state_gt}

    def sample(self, *a, **k):
        raise NotImplementedError("the h -> u DDIM sampler (models/ddim.py:706-806) is not built; PlDdim's evaluation loops "
                                  "use sample_with_repeat / sample_edm")

    def sample_with_repeat(self, h, u, sparams, return_last=True, guide_dx=False):
        """models/ddim.py:808-913: DDIM steps (eta, uniform / quad skipping) with n_repeat RePaint-style inner loops per step
        and the previous x0 prediction fed back as x_self_cond; the loop runs in mcedm_ddim_repaint_sample (csrc/ddpm.hip).
        h, u: 'b h w c' normalised fields.  Returns (xs, x0_preds), fp32 'b t h w c' like the reference.
        With eta != 0 the per-step torch.rand_like of :893 (a UNIFORM draw) is generated inside the step kernel from a seed drawn
        from torch's CPU generator (``noise_source`` "device", also when the attribute is absent), or made up front as one
        torch.rand([S, B, C, H, W]) (``"torch"``).  Either way the call replays from one HIP graph."""
        if guide_dx:
            raise NotImplementedError("guide_dx=True (PDE guidance) is outside the built path")
        noise_source = self._noise_mode()
        net = self._net(self.ema_model if self.ema_model is not None else self.model)
        hu = _nchw(torch.cat([h, u], dim=-1)).float()
        ae = self._alphas_ext()
        dd, keep = _lib.ddim_desc(sparams, ae, self.h_ch, self.u_ch, net.self_condition)
        hu_noise = torch.randn_like(hu)
        stochastic = abs(float(sparams.eta)) > 1e-10
        dev_noise = stochastic and noise_source == "device"
        eta_noise = None
        if stochastic and not dev_noise:           # the reference draws torch.rand_like (UNIFORM) here, models/ddim.py:893
            S = len(range(0, self.num_timesteps, self.num_timesteps // dd.timesteps)) if dd.skip_type == 0 else dd.timesteps
            eta_noise = torch.rand((S,) + tuple(hu.shape), dtype=torch.float32, device=hu.device)
        kw = dict(seed=self._draw_seed()) if dev_noise else {}
        with torch.no_grad():
            packed = net.packed_weights()
            eager = lambda x, nz, en, seed=None: net.plan.ddim_repaint_sample(      # noqa: E731
                packed, dd, x, nz, en, return_last=return_last, ws=self._sample_ws, rng_seed=self._seed_tensor(seed, x.device))
            B = hu.shape[0]
            key = ("ddim", B, bool(return_last), stochastic, dev_noise, packed.data_ptr(), hu.device.index, _table_key(ae),
                   _lib.desc_key(dd, skip=("alphas_cumprod_ext",)))
            return self._replay(key, lambda: _lib.GraphedDdimRepaint(net.plan, packed, dd, keep, B, stochastic, return_last,
                                                                     ws=self._sample_ws, device_noise=dev_noise),
                                eager, hu, hu_noise, eta_noise, **kw)

    def _no_backward(self):
        if torch.is_grad_enabled():
            raise NotImplementedError("DDPM (epsilon-prediction) training is not built: SURVEY.md section 8 f1 covers EDM sampling "
                                      "of a trained DDPM checkpoint (Model has no backward here).  Under torch.no_grad() forward and "
                                      "training_step run: the noising pass and the loss value, without gradients")

    def forward(self, x, t, noise, cond=None):
        """models/ddim.py:195-226 without gradients: (output, x0_t), one timestep per sample."""
        self._no_backward()
        return self._ddpm_eps_forward(x, t, noise, cond)

    def training_step(self, *a, **k):
        """training_step(train_batch, batch_idx), models/ddim.py:264-292, under torch.no_grad(): the noise-estimation loss of the
        batch (logged as train_loss), no gradients."""
        self._no_backward()
        train_batch = a[0] if a else k["train_batch"]
        if self.pde_loss_lambda:
            raise NotImplementedError("pde_loss_lambda > 0 (models/ddim.py:284-290) is not built")
        h_unnorm, dx, dt, u_unnorm = train_batch
        self.h_ch, self.u_ch = h_unnorm.shape[-1], u_unnorm.shape[-1]
        x = _nchw(self.data_transform(h_unnorm, u_unnorm)).float()
        n = x.size(0)
        noise = torch.randn_like(x)
        t = torch.randint(low=0, high=self.num_timesteps, size=(n // 2 + 1,))       # antithetic sampling (:275-278)
        t = t.to(x.device).long()
        t = torch.cat([t, self.num_timesteps - t - 1], dim=0)[:n]
        return self._ddpm_eps_loss(self.forward(x, t, noise)[0], noise)


def _eps_train_loss(module, x_noise, labels, cond, noise, dx=None):
    """NoiseEstimationLoss of PlCondDdim.training_step (models/ddim.py:1118-1152, models/losses.py:39-59):
    loss = mean_b sum_chw (F - noise)^2 with F = model(x_noise, t.float(), cond').  Forward and backward run in the HIP library
    (mcedm_unet_forward, mcedm_eps_loss, mcedm_unet_backward; with dx_cond mcedm_unet_forward_dx and mcedm_unet_backward_dx, dx
    being the network's dx input of this batch or None)."""
    net: DhariwalUNet = module.model
    net.arm_dropout(module._draw_seed)      # dropout in train() mode: this step's seed, after the reference's own draws

    def run():
        F = net.plan.forward(net.packed_weights(), x_noise, labels, cond=cond, ws=module._train_ws, training=True, dx=dx)
        loss, dF = _lib.eps_loss(F, noise, want_grad=True)
        return loss, lambda grads: net.plan.unet_backward(net.packed_weights(), net.named_param_dict(), x_noise, labels, cond, dF,
                                                          grads, ws=module._train_ws, dx=dx)
    return _TrainLoss.apply(module, run, *net.parameters())


class PlCondDdim(_DdpmSchedule, _SingleTask):
    """models/ddim.py:1053-1605: the single-task conditional DDPM (epsilon prediction) on the ADM U-Net
    (configs/model/adm_cond_h_res32.yaml: ``name: adm_cond_h``, ``self_cond: True``, ``cond_p: 1.``), trained with the noise
    estimation loss and sampled with the EDM Heun sampler around VP preconditioning (``get_denoised``, :915-947).

    Constructor, buffers (``betas``, ``logvar``), state_dict keys and method signatures follow the reference.  The training
    step runs in the HIP library: noising (mcedm_eps_noise_inputs), the self-conditioning pre-pass and its estimate written into
    the network's widened conditioning input (mcedm_eps_self_cond), forward, loss (mcedm_eps_loss) and backward from dF
    (mcedm_unet_backward); ``sample_edm`` is mcedm_vp_heun_sample[_rng].  The PDE loss term raises.  ``dx_cond`` (with ``dx_norm:
    prob``, the one normalisation the reference can run; ``cat_dx`` True or False) runs on the ADM U-Net: training draws the dx
    switch first, evaluates the residual gradient on the noised target from the cond before the ``cond_p`` drop and feeds it to the
    pre-pass and the main pass (mcedm_unet_forward_dx / mcedm_unet_backward_dx); ``sample`` and ``sample_edm`` evaluate it on the
    device at every network evaluation (mcedm_cond_ddim_sample_dxcond: unscaled; mcedm_vp_heun_sample_dxcond: scaled by c_in), with
    ``guide_dx`` on top if asked; it refuses what ``guide_dx`` refuses.
    ``sample`` (the DDIM loop, :1452-1530) is mcedm_cond_ddim_sample[_rng].  ``guide_dx=True`` (PDE guidance, :1499-1503 and
    :1576-1590) runs in both samplers on both networks (mcedm_[ddpm_]cond_ddim_sample_guided, mcedm_[ddpm_]vp_heun_sample_guided) for
    scalar gauss-normalised fields with h given on the device; every other form of it raises.

    With a ``name`` that does not start with ``adm`` the network is the DDPM U-Net ``Model`` (:43-46;
    configs/model/ddim_cond_h_res32.yaml: ``name: ddim_cond_h``, ``cat_cond: False``, ``self_cond: True``) with its cond_enc head,
    for EVALUATION: ``get_denoised``, ``sample_edm``, ``sample``, ``validation_step`` and ``test_step`` run on it
    (mcedm_ddpm_vp_heun_sample[_rng], mcedm_ddpm_cond_ddim_sample[_rng]).  ``Model`` has no backward here: with gradients enabled
    ``training_step`` and ``forward`` raise; under ``torch.no_grad()`` they run with one timestep per sample (mcedm_ddpm_forward_t)
    and return the reference's ``(output, x0_t)`` and loss value.  ``noise_source`` ("device" / "torch", from MCEDM_NOISE_SOURCE) says where the per-step draws of
    the two samplers come from: the sampler's own kernels, or torch tensors drawn up front."""

    def __init__(self, hparams):
        super().__init__()
        self.save_hyperparameters()
        m, o = hparams.model, hparams.optimization
        self._on_ddpm_unet = not str(hparams.name).startswith("adm")                    # models/ddim.py:43-46
        # dx_cond (models/ddim.py:33-35, 199-204): as for PlCondEdm only dx_norm == 'prob' can run in the reference (pinned:
        # tests/golden/cond_ddim_dx_cat.npz 'dx_norm_l2_raises'), so the other normalisations raise here as well
        self.dx_cond = bool(_opt(m, "dx_cond", False))
        self.dx_norm, self.dx_detach = _opt(m, "dx_norm", "l2"), _opt(m, "dx_detach", False)
        if self.dx_cond and self.dx_norm != "prob":
            raise NotImplementedError(f"dx_cond with dx_norm={self.dx_norm!r}: PlCondDdim.get_dx_input raises in the reference for "
                                      "every dx_norm other than 'prob' (models/ddim.py:608-611, 1445-1448)")
        if self.dx_cond and self._on_ddpm_unet:
            raise NotImplementedError("dx_cond (models/ddim.py:33-35) is not built on the DDPM U-Net")
        if _opt(o, "pde_loss_lambda", 0.0):
            raise NotImplementedError("pde_loss_lambda > 0 (models/ddim.py:1144-1150) is not built")
        self.node_type = bool(_opt(m, "node_type", False))
        if self.node_type:
            m.cond_channels = m.cond_channels + 1
        self._register_schedule(hparams)
        if self._on_ddpm_unet:
            if _opt(m, "cat_cond", False) and _opt(m, "cond_channels", 0) > 0:
                raise NotImplementedError("cat_cond on the DDPM U-Net (models/ddim_blocks.py:259, 386-391) is not built for PlCondDdim: "
                                          "its VP preconditioning scales the concatenated cond (models/ddim.py:932); no shipped "
                                          "configuration uses it (PlCondEdm runs cat_cond on this network)")
            from .ddim_blocks import Model
        self.model = Model(hparams) if self._on_ddpm_unet else DhariwalUNet(hparams)
        self.ema_model = EmaModel(self.model, beta=m.ema_rate) if m.ema else None
        self.cond_p = _opt(m, "cond_p", 0.8)                                           # models/ddim.py:1058
        self._init_common(hparams, m.in_channels, m.out_ch)
        self.factor, self.step_size, self.loss = _opt(o, "factor", 0.3), _opt(o, "step_size", 50), _opt(o, "loss", "l2")
        self.pde_loss_lambda = 0.0
        self.edm_steps = self.sigma_min = self.sigma_max = None
        self.noise_source = os.environ.get("MCEDM_NOISE_SOURCE", "device")      # the samplers' per-step draws, as in PlMcedm
        self.h_ch, self.u_ch = m.cond_channels - (1 if self.node_type else 0), m.out_ch
        self._tables = None
        self._stage = None

    # ---- epsilon-prediction forward (models/ddim.py:195-226) --------------------------------------------------------------
    def _noised_inputs(self, x, t, noise, cond, ws):
        """x_noise, labels, the network's conditioning input, t and dx of one forward, consuming torch's generator as the reference
        does: with dx_cond the dx draw first (:199, only then), the cond_p draw (:202), then the self-conditioning draw (:205)
        whose pre-pass runs in `ws` before anything else uses it.  dx = get_dx_input(cond[:, 0:h_ch], x_noise) is taken from the
        cond BEFORE the cond_p drop, on the noised target, and goes to the pre-pass and the main pass alike (:216, :220)."""
        net = self.model
        x = x.to(torch.float32).contiguous()
        noise = noise.to(torch.float32).contiguous()
        t = torch.as_tensor(t).to(device=x.device, dtype=torch.int64).reshape(-1).contiguous()
        sa, sb = self._noise_tables(x.device)
        x_noise, labels = _lib.eps_noise_inputs(x, noise, t, sa, sb)
        dx = None
        if self.dx_cond and torch.rand(1) > 0.1:           # dx off with a small probability; it carries no gradient
            dx = self._dx_train_input(cond, x_noise)
        if torch.rand(1) >= self.cond_p:
            cond = None                                    # the conditioning switched off for this batch
        cond = None if cond is None else cond.to(torch.float32).contiguous()
        if not net.self_condition:
            return x_noise, labels, cond, t, dx
        B, _, H, W = x.shape
        shape = (B, net.plan_cond_channels, H, W)
        if self._stage is None or tuple(self._stage.shape) != shape or self._stage.device != x.device:
            self._stage = torch.empty(shape, dtype=torch.float32, device=x.device)
        stage = self._stage
        if torch.rand(1) < 0.5:                            # no-grad pre-pass: F0 = model(x_noise, t, cond)
            pk = net.packed_weights()
            pre_cond = _lib.eps_self_cond(stage, cond, net.cond_channels, net.state_channels) if cond is not None else None
            F0 = net.plan.forward(pk, x_noise, labels, cond=pre_cond, ws=ws, dx=dx)
            _lib.eps_self_cond(stage, cond, net.cond_channels, net.state_channels, x_noise=x_noise, F0=F0, t=t, sqrt_ab=sa,
                               sqrt_1mab=sb)
            return x_noise, labels, stage, t, dx
        if cond is None:
            return x_noise, labels, None, t, dx
        return x_noise, labels, _lib.eps_self_cond(stage, cond, net.cond_channels, net.state_channels), t, dx

    def _dx_train_input(self, cond, x_noise):
        """get_dx_input(cond[:, 0:h_ch], x_noise) of forward (:200-201) under the refusals of the samplers' dx path."""
        if cond is None:
            raise NotImplementedError("dx_cond needs the conditioning field: forward without cond is not built")
        self._dx_check()
        with torch.no_grad():
            return self.get_dx_input(cond[:, 0:self.h_ch], x_noise)

    def forward(self, x, t, noise, cond=None):
        """models/ddim.py:195-226 without gradients: (output, x0_t)."""
        self._adm_only("forward (the noising pass of training)")
        if self._on_ddpm_unet:
            return self._ddpm_eps_forward(x, t, noise, cond)
        net = self.model
        with torch.no_grad():
            x_noise, labels, condp, t, dx = self._noised_inputs(x, t, noise, cond, net._ws)
            output = net.plan.forward(net.packed_weights(), x_noise, labels, cond=condp, ws=net._ws, dx=dx)
            sa, sb = self._noise_tables(x.device)
            x0_t = torch.empty_like(output)
            _lib.eps_self_cond(x0_t, None, 0, output.shape[1], x_noise=x_noise, F0=output, t=t, sqrt_ab=sa, sqrt_1mab=sb)
        return output, x0_t

    def training_step(self, train_batch, batch_idx):
        self._adm_only("training_step")
        h_unnorm, dx, dt, u_unnorm = train_batch
        self.h_ch, self.u_ch = h_ch, u_ch = h_unnorm.shape[-1], u_unnorm.shape[-1]
        x = self.data_transform(h_unnorm, u_unnorm)
        n = x.size(0)
        h, u = x[..., 0:h_ch], x[..., h_ch:h_ch + u_ch]
        cond_in = _nchw(self.get_cond_in(h, u, dx, dt)).float()
        u = _nchw(u).float()
        noise = torch.randn_like(u)
        t = torch.randint(low=0, high=self.num_timesteps, size=(n // 2 + 1,))       # antithetic sampling (:1134-1137)
        t = t.to(x.device).long()
        t = torch.cat([t, self.num_timesteps - t - 1], dim=0)[:n]
        if self._on_ddpm_unet:                       # under torch.no_grad() (see _adm_only): the loss value alone
            return self._ddpm_eps_loss(self._ddpm_eps_forward(u, t, noise, cond_in)[0], noise)
        x_noise, labels, condp, _, dx_in = self._noised_inputs(u, t, noise, cond_in, self._train_ws)
        loss = _eps_train_loss(self, x_noise, labels, condp, noise.contiguous(), dx_in)
        self.log("train_loss", loss, prog_bar=True, on_epoch=True, on_step=False, sync_dist=True)
        return loss

    # ---- sampling (models/ddim.py:915-957, 1532-1605) ---------------------------------------------------------------------
    def get_self_cond_edm(self, denoised):
        return None                                        # :1603-1605

    def _c_noise(self, sigma):
        return float(self.num_timesteps - 1 - self.round_sigma(torch.tensor([float(sigma)], dtype=torch.float32),
                                                               return_index=True).to(torch.float32)[0])

    def get_denoised(self, model, xt, t, cond=None, x_self_cond=None, dx=None, w=None):
        """models/ddim.py:915-947 at one noise level (the sampler's case): one VP-preconditioned Heun step's denoiser call,
        run as a single-step mcedm_vp_heun_sample would; here through the network directly: D = x - sigma F(c_in x, c_noise,
        c_in cond)."""
        if self.edm_steps is None:
            raise RuntimeError("call set_test_sampler_params(params) with params.type == 'edm' first (models/ddim.py:122-129)")
        net = self._net(model)
        if dx is not None and (self._on_ddpm_unet or not net.dx_cond):
            raise NotImplementedError("dx given to a network built without dx_cond (models/ddim.py:933-934); dx_cond is not built "
                                      "on the DDPM U-Net")
        sig = torch.as_tensor(t).reshape(-1)
        if sig.numel() != 1:
            raise NotImplementedError("one noise level for the whole batch (what sample_edm evaluates)")
        s32 = float(sig.to(torch.float32)[0])
        c_in = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(s32 * s32 + 1.0, dtype=torch.float32).sqrt()
        c_in_dev = c_in.reshape(1).to(xt.device)
        labels = torch.full((1,), self._c_noise(s32), dtype=torch.float32, device=xt.device)
        xt = xt.to(torch.float32).contiguous()
        B, _, H, W = xt.shape
        with torch.no_grad():
            pk = net.packed_weights()
            if self._on_ddpm_unet:     # cond is not scaled (cat_condition False, :932): its map once, for both evaluations
                t_lab = float(labels[0])
                cmap = None if cond is None else net.plan.cond_map(pk, cond.to(torch.float32).contiguous())
                x_in = (c_in_dev * xt).contiguous()
                xsc = None if x_self_cond is None else (c_in_dev * x_self_cond.to(torch.float32)).contiguous()
                F = net.plan.forward_cond(pk, x_in, t_lab, cond_map=cmap, x_self_cond=xsc, ws=net._ws)
                if not (w is None or abs(w) < 0.001 or cond is None):
                    F = (w + 1) * F - w * net.plan.forward_cond(pk, x_in, t_lab, x_self_cond=xsc, ws=net._ws)
                return xt + (-c_in.new_tensor(s32).to(xt.device)) * F, F

            def evaluate(c, sc, d=None):
                # the conv_in rows scale every input channel by c_in: x, cond, x_self_cond and dx (:921-935)
                cp = net.stage_self_cond(None if c is None else (c_in_dev * c).contiguous(),
                                         None if sc is None else (c_in_dev * sc).contiguous(), xt) \
                    if net.self_condition else (None if c is None else (c_in_dev * c).contiguous())
                return net.plan.forward(pk, (c_in_dev * xt).contiguous(), labels, cond=cp, ws=net._ws,
                                        dx=None if d is None else (c_in_dev * d).to(torch.float32).contiguous())
            c32 = None if cond is None else cond.to(torch.float32)
            F = evaluate(c32, x_self_cond, dx)
            # :938-942: the branch is taken when cond OR dx is given; its second evaluation drops both
            if not (w is None or abs(w) < 0.001 or (cond is None and dx is None)):
                F = (w + 1) * F - w * evaluate(None, x_self_cond)
            D = xt + (-c_in.new_tensor(s32).to(xt.device)) * F
        return D, F

    def _guidance(self, h, guide_dx):
        """The residual description of guide_dx=True (None without it), as PlCondEdm.sample_edm builds it; h 'b h w c'."""
        if not guide_dx:
            return None
        if h is None or not getattr(h, "is_cuda", False):
            raise NotImplementedError("guide_dx (PDE guidance, models/ddim.py:1501-1503, 1576-1590) needs the conditioning field h on "
                                      "the device: guidance without it, or off the device, is not built")
        if self.pde_loss is None or not hasattr(self.pde_loss, "guidance_desc"):
            raise NotImplementedError("guide_dx needs set_pde_loss_function('swe' | 'swe_per' | 'darcy')")
        if self.rescaled or self.normalization == "min_max" or self.h_ch != 1 or self.u_ch != 1:
            raise NotImplementedError("guide_dx is built for scalar gauss-normalised fields h, u")
        return self.pde_loss.guidance_desc(self.normalizer_input, self.normalizer_target, h.shape[1], h.shape[2])

    def _dx_check(self):
        """What dx_cond refuses, in training and in both samplers: what the guided path refuses."""
        if self.pde_loss is None or not hasattr(self.pde_loss, "guidance_desc"):
            raise NotImplementedError("dx_cond needs set_pde_loss_function('swe' | 'swe_per' | 'darcy')")
        if self.rescaled or self.normalization == "min_max" or self.h_ch != 1 or self.u_ch != 1:
            raise NotImplementedError("dx_cond is built for scalar gauss-normalised fields h, u")

    def _dx_input(self, h):
        """The description of the residual whose gradient at the sampler's current state is the network's dx input (None for a
        module without dx_cond); h 'b h w c'."""
        if not self.dx_cond:
            return None
        if h is None or not getattr(h, "is_cuda", False):
            raise NotImplementedError("dx_cond (models/ddim.py:1492, 1571, 1584) needs the conditioning field h on the device: "
                                      "sampling without it, or off the device, is not built")
        self._dx_check()
        return self.pde_loss.guidance_desc(self.normalizer_input, self.normalizer_target, h.shape[1], h.shape[2])

    def sample_edm(self, h, u_noise, sparams, return_last=True, guide_dx=False):
        """models/ddim.py:1532-1601; h, u_noise in the reference's 'b h w c' layout; returns [b, t, h, w, c] float64.  The
        schedule is rounded on the host (round_sigma, :1553, 1566); the loop runs in mcedm_vp_heun_sample_rng, whose churn kernel
        generates the per-step randn_like(x_cur) of :1567 from a seed drawn from torch's CPU generator (``noise_source =
        "device"``), or in mcedm_vp_heun_sample fed one torch.randn([N, B, C, H, W], float64) (``"torch"``).  Either way the call
        replays from one HIP graph.  guide_dx=True: after every denoiser call d -= 5 * dx / t_hat with dx the PDE-residual gradient
        at the denoised state (:1576-1578, 1589-1590), evaluated on the device (mcedm_[ddpm_]vp_heun_sample_guided)."""
        guidance, dx_input = self._guidance(h, guide_dx), self._dx_input(h)
        noise_source = self._noise_mode()
        if self.edm_steps is None:
            self.set_test_sampler_params(sparams)
        net = self._net(self.ema_model if self.ema_model is not None else self.model)
        h, init = _nchw(h).float().contiguous(), _nchw(u_noise).float().contiguous()
        N, t_steps, t_hat, c_noise = self._edm_schedule(sparams, lambda t: self._c_noise(float(t)))
        vd = _lib.vp_sampler_desc(N, net.cond_channels, t_steps.tolist(), t_hat, c_noise, float(sparams.S_noise), float(sparams.w))
        churn = any(th != float(t_steps[i]) for i, th in enumerate(t_hat))     # the steps whose x_hat adds noise (:1567)
        dev_noise = churn and noise_source == "device"
        step_noise = None
        if noise_source == "torch":                # drawn whether or not a step churns, like the reference's randn_like
            step_noise = torch.randn((N,) + tuple(init.shape), dtype=torch.float64, device=init.device)
            if not churn:
                step_noise = None                  # nothing reads it
        kw = dict(seed=self._draw_seed()) if dev_noise else {}
        cond = h if net.cond_channels > 0 else None
        # dx_cond: dx_in = get_dx_input(h, x) in front of every get_denoised (:1571, 1584), inside mcedm_vp_heun_sample_dxcond
        dxkw = {} if dx_input is None else dict(dx_input=dx_input)
        dxkey = () if dx_input is None else (_lib.desc_key(dx_input),)
        with torch.no_grad():
            packed = net.packed_weights()
            eager = lambda c, i, sn, seed=None: net.plan.vp_sample(      # noqa: E731
                packed, vd, c, i, sn, return_last=return_last, ws=self._sample_ws, rng_seed=self._seed_tensor(seed, i.device),
                guidance=guidance, **dxkw)
            # the residual descriptions of guide_dx and dx_cond are host-side structs: part of the key and of the capture
            B, _, H, W = init.shape
            key = ("vp", B, H, W, bool(return_last), churn, dev_noise, packed.data_ptr(), init.device.index, N, net.cond_channels,
                   tuple(t_steps.tolist()), tuple(t_hat), tuple(c_noise), float(sparams.S_noise), float(sparams.w),
                   None if guidance is None else _lib.desc_key(guidance)) + dxkey
            return self._replay(key, lambda: _lib.GraphedVpSampler(net.plan, packed, vd, B, H, W, cond is not None, churn,
                                                                   return_last=return_last, ws=self._sample_ws,
                                                                   device_noise=dev_noise, guidance=guidance, **dxkw),
                                eager, cond, init, step_noise, **kw)

    def sample(self, *a, **k):
        """``sample(h, u_noise, sparams, return_last=True, guide_dx=False)`` of models/ddim.py:1452-1530 (the open signature is the
        one the stub had, which tests/test_pl_layout_cpu.py pins; the arguments are bound by ``_ddim_sample``)."""
        return self._ddim_sample(*a, **k)

    def _ddim_sample(self, h, u_noise, sparams, return_last=True, guide_dx=False):
        """models/ddim.py:1452-1530, the DDIM sampler (``type: ddim``, the reference's default sampler configuration): h, u_noise
        in the reference's 'b h w c' layout; returns (xs, x0_preds), fp32 'b t h w c'.  The loop runs in mcedm_cond_ddim_sample:
        per step one network pass (two with classifier-free guidance, |w| >= 0.001) and one fused kernel that also feeds the
        x0 prediction back as the next step's x_self_cond.  With eta != 0 the per-step torch.rand_like(x) of :1512 (a UNIFORM
        draw) is generated inside that kernel from a seed drawn from torch's CPU generator (``noise_source = "device"``), or made
        up front as one torch.rand([S, B, C, H, W]) (``"torch"``).  guide_dx=True: et -= 5 * sqrt(1 - at) * dx with dx the
        PDE-residual gradient at each step's noisy state xt (:1501-1503), evaluated on the device in front of the step's network
        passes (mcedm_[ddpm_]cond_ddim_sample_guided)."""
        guidance = self._guidance(h, guide_dx)
        dx_input = None if h is None else self._dx_input(h)
        if h is None:
            raise NotImplementedError("sampling without the conditioning field h (models/ddim.py:1452-1531 hands cond=h to the "
                                      "network in every step) is not built")
        noise_source = self._noise_mode()
        net = self._net(self.ema_model if self.ema_model is not None else self.model)
        h, init = _nchw(h).float().contiguous(), _nchw(u_noise).float().contiguous()
        ae = self._alphas_ext()
        dd = _lib.cond_ddim_desc(sparams, ae, net.cond_channels, self._net(self.model).self_condition)
        stochastic = abs(float(sparams.eta)) > 1e-10
        dev_noise = stochastic and noise_source == "device"
        S = len(_lib.ddim_timesteps(self.num_timesteps, dd.timesteps, dd.skip_type))
        eta_noise = (torch.rand((S,) + tuple(init.shape), dtype=torch.float32, device=init.device)
                     if stochastic and not dev_noise else None)
        kw = dict(seed=self._draw_seed()) if dev_noise else {}
        cond = h if net.cond_channels > 0 else None
        # dx_cond: dx_in = get_dx_input(h, xt) at every step's noisy state (:1492), inside mcedm_cond_ddim_sample_dxcond
        dxkw = {} if dx_input is None else dict(dx_input=dx_input)
        dxkey = () if dx_input is None else (_lib.desc_key(dx_input),)
        with torch.no_grad():
            packed = net.packed_weights()
            eager = lambda c, i, en, seed=None: net.plan.cond_ddim_sample(      # noqa: E731
                packed, dd, c, i, en, return_last=return_last, ws=self._sample_ws, rng_seed=self._seed_tensor(seed, i.device),
                guidance=guidance, **dxkw)
            # the evaluation loops repeat the call: it replays from one HIP graph, like sample_edm of the sibling modules
            B, _, H, W = init.shape
            key = ("ddim", B, H, W, bool(return_last), stochastic, dev_noise, packed.data_ptr(), init.device.index, _table_key(ae),
                   _lib.desc_key(dd, skip=("alphas_cumprod_ext",)), None if guidance is None else _lib.desc_key(guidance)) + dxkey
            return self._replay(key, lambda: _lib.GraphedCondDdim(net.plan, packed, dd, B, H, W, stochastic, return_last=return_last,
                                                                  ws=self._sample_ws, device_noise=dev_noise, guidance=guidance,
                                                                  **dxkw),
                                eager, cond, init, eta_noise, **kw)
