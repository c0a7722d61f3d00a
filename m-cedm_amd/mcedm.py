"""Drop-in ``PlMcedm`` for the reference's ``models/mcedm.py`` (M-CEDM LightningModule).

Same constructor (``PlMcedm(hparams)``), attributes, state_dict keys and method signatures as the
reference (models/mcedm.py:16-639): Hydra can instantiate it with ``_target_`` pointed here and
Lightning drives ``training_step`` / ``validation_step`` / ``test_step`` unchanged.  Everything from
``model_precond`` / ``get_denoised`` / ``sample_edm`` / the training loss downwards runs in
libmcedm_hip.so; the metric bookkeeping around it (MAE, PDE residual, return dicts for the plotting
callbacks) stays in Python like the reference's.

``Normalizer``, ``DotDict``, ``masked_l1`` and everything else the drop-ins for ``models/ddim.py`` need as well live in
``m-cedm_amd/pl_base.py`` and are re-exported here.

Deliberate differences, all documented in INTEGRATION.md:
  * sample_edm draws the per-step churn noise only for steps with gamma > 0 (the reference draws and
    multiplies by zero otherwise, mcedm.py:608), so device RNG streams differ for S_churn = 0;
  * guide_dx=True raises: the reference's joint-model guidance hook itself raises (models/mcedm.py:500-518 slices the
    wrong axis); PDE guidance runs on the device for the single-task sampler (mcedm_amd.ddim.PlCondEdm).  dx_cond of the JOINT
    model goes through the same failing hook in the reference (get_dx_input -> get_dx_pde, models/mcedm.py:519-526), so it is
    rejected here; the dx-conditioned network itself is built and runs for the single-task model (mcedm_amd.ddim.PlCondEdm).
"""
from __future__ import annotations

import os

import torch

from . import lib as _lib
from .adm_blocks import DhariwalUNet, EmaModel
from .pl_base import (DotDict, Normalizer, _Base, _PlBase, _TrainLoss, _ddim_sampler_params, _nchw, _opt,  # noqa: F401
                      masked_l1)


def _edm_train_loss(module, x, x_noise, sigma, cond, mask, dx, extra=None):
    """loss = mean_b sum_chw w(sigma_b) (D*m - x*m)^2 with D = model_precond(x_noise, sigma, cond): forward and
    backward both run in the HIP library (mcedm_edm_denoise / mcedm_edm_loss / mcedm_edm_denoise_backward).
    dx: the network's PDE-gradient input of dx_cond models (PlCondEdm.training_step) or None; no gradient flows into it.
    extra(D, dD, loss) -> loss: a further term of the loss in D (the PDE residual of PlCondEdm.training_step); it adds its
    gradient to dD in place and returns the total, and the backward from dD is the same."""
    net: DhariwalUNet = module.model
    # hparams.model.dropout in train() mode: one seed per step, drawn AFTER the reference's own draws of the step (noise,
    # rnd_normal, the dx / cond_p torch.rand's), so a dropout = 0 run with the same torch.manual_seed sees the same data noise
    net.arm_dropout(module._draw_seed)

    def run():
        D = net.plan.denoise(net.packed_weights(), x_noise, sigma, cond=cond, ws=module._train_ws, training=True,
                             sigma_data=module.sigma_data, dx=dx)
        loss, dD = _lib.edm_loss(D, x, mask, sigma, sigma_data=module.sigma_data, want_grad=True)
        if extra is not None:
            loss = extra(D, dD, loss)
        return loss, lambda grads: net.plan.denoise_backward(
            net.packed_weights(), net.named_param_dict(), x_noise, sigma, cond, dD, grads, ws=module._train_ws,
            sigma_data=module.sigma_data, dx=dx)
    return _TrainLoss.apply(module, run, *net.parameters())


class PlMcedm(_PlBase):
    def __init__(self, hparams):
        super().__init__()
        self.save_hyperparameters()
        m, o = hparams.model, hparams.optimization
        self.cond_p = 1.0
        if _opt(m, "dx_cond", False):
            raise NotImplementedError("hparams.model.dx_cond=True cannot run for the joint model in the reference either "
                                      "(PlMcedm.get_dx_pde slices the wrong axis, models/mcedm.py:500-518); see DESIGN.md")
        if not str(hparams.name).startswith("adm"):
            raise NotImplementedError("only the ADM/EDM U-Net (hparams.name = 'adm*') is on the hot path")
        self.dx_cond = False
        if _opt(m, "self_cond", False):
            raise NotImplementedError("hparams.model.self_cond=True is outside the MI355X hot path for PlMcedm")
        # models/mcedm.py:25-34: the two optional widenings of the conditioning input.  Like the reference, the constructor
        # rewrites hparams.model.cond_channels before the network is built (the C ABI takes any cond_channels).
        self.add_cond_mask, self.add_xt = bool(_opt(m, "add_cond_mask", False)), bool(_opt(m, "add_xt", False))
        if self.add_cond_mask:
            m.cond_channels = m.cond_channels + m.in_channels          # the observation mask rides along (SSSD-S4 style)
        if self.add_xt:
            m.cond_channels = m.cond_channels + 2                      # the grid coordinates dx, dt
        self.model = DhariwalUNet(hparams)
        self.ema_model = EmaModel(self.model, beta=m.ema_rate) if m.ema else None
        # EDM preconditioning constants (mcedm.py:45-50)
        self.P_mean, self.P_std, self.sigma_data = -1.2, 1.2, 1.0
        self.sigma_min, self.sigma_max = 0.002, 80
        self.factor, self.step_size, self.loss = o.factor, o.step_size, o.loss
        # models/mcedm.py:72-76 reads the three knobs and the joint model's training_step (:254-281) never uses them: accepted and
        # ignored here as well
        self.pde_loss_lambda = _opt(o, "pde_loss_lambda", 0.0)
        self.pde_loss_prop_t = _opt(o, "pde_loss_prop_t", False)
        self.use_gt_pde = _opt(o, "use_gt_pde", False)
        self.h_ch = self.u_ch = m.out_ch // 2
        self._init_common(hparams, self.h_ch, self.u_ch)
        # where the sampler's per-step churn noise (models/mcedm.py:608) comes from: "device" = generated inside the kernel that
        # applies it (mcedm_heun_sample_rng; keyed by a seed drawn from torch's CPU generator, so seed_everything still pins a
        # run), "torch" = torch.randn((N, B, 2, H, W), float64) materialised up front (2.1 GB at the reference's shipped
        # 50-step / n_samples 5 config and 32 inputs; what the golden vectors inject)
        self.noise_source = os.environ.get("MCEDM_NOISE_SOURCE", "device")

    # ---- configuration hooks (same names as the reference) ------------------------------------------
    @staticmethod
    def get_sampler_params(params):
        return _ddim_sampler_params() if params.get("sampler", None) is None else params.sampler

    def set_test_sampler_params(self, params):
        self.test_sparams = params

    def get_loss_weight(self, sigma):
        return (sigma ** 2 + self.sigma_data ** 2) / (sigma * self.sigma_data) ** 2

    def get_cond_in(self, x, mask, dx=None, dt=None):
        """models/mcedm.py:241-252 ('b h w c' tensors): observed values, noise where the state is missing -- or, with
        add_cond_mask, zeros there plus the observation mask as extra channels; add_xt appends the batch's dx / dt fields."""
        if self.add_cond_mask:
            cond_in = torch.cat([x * (1 - mask), (1. - mask)], dim=-1)
        else:
            cond_in = x * (1 - mask) + torch.randn_like(x) * mask
        if self.add_xt:
            cond_in = torch.cat([cond_in, dx, dt], dim=-1)
        return cond_in

    # ---- preconditioned network (HIP) ------------------------------------------------------------------
    def model_precond(self, x_noise, sigma, cond=None, x_self_cond=None, dx=None):
        if x_self_cond is not None or dx is not None:
            raise NotImplementedError("x_self_cond / dx are outside the hot path")
        net = self.model
        with torch.no_grad():
            return net.plan.denoise(net.packed_weights(), x_noise.float().contiguous(),
                                    sigma.to(torch.float32).reshape(-1).contiguous(),
                                    cond=None if cond is None else cond.float().contiguous(), ws=net._ws,
                                    sigma_data=self.sigma_data)

    def get_denoised(self, model, xt, t, cond=None, x_self_cond=None, dx=None, w=None):
        if x_self_cond is not None or dx is not None:
            raise NotImplementedError("x_self_cond / dx are outside the hot path")
        net = self._net(model)
        xt = xt.to(torch.float32).contiguous()
        sigma = torch.as_tensor(t).to(torch.float32).reshape(-1).contiguous().to(xt.device)
        cond = None if cond is None else cond.float().contiguous()
        packed = net.packed_weights()
        with torch.no_grad():
            D, F = net.plan.denoise(packed, xt, sigma, cond=cond, ws=net._ws, sigma_data=self.sigma_data, want_F=True)
            if not (w is None or abs(w) < 0.001 or cond is None):          # classifier-free blend, mcedm.py:453-458
                _, Fu = net.plan.denoise(packed, xt, sigma, cond=None, ws=net._ws, sigma_data=self.sigma_data, want_F=True)
                D, F = self._cfg_blend(xt, sigma, F, Fu, w)
        return D, F

    def round_sigma(self, sigma, return_index=False):
        return 0 if return_index else torch.as_tensor(sigma)

    def forward(self, x, sigma, noise, cond=None, mask=None):
        x_noise = x + (mask * noise * sigma if mask is not None else noise * sigma)
        if torch.rand(1) >= self.cond_p:
            cond = None
        return self.model_precond(x_noise, sigma.float(), cond)

    # ---- training ------------------------------------------------------------------------------------
    def training_step(self, train_batch, batch_idx):
        h_unnorm, dx, dt, u_unnorm, mask = train_batch
        self.h_ch, self.u_ch = h_unnorm.shape[-1], u_unnorm.shape[-1]
        x = self.data_transform(h_unnorm, u_unnorm)                       # b h w c
        cond_in = _nchw(self.get_cond_in(x, mask, dx, dt))
        x = _nchw(x)
        noise = torch.randn_like(x)
        rnd_normal = torch.randn([x.shape[0], 1, 1, 1]).type_as(x)        # CPU generator, like mcedm.py:269-270
        mask_c = _nchw(mask).to(torch.float32)
        x_noise, sigma = _lib.edm_noise_inputs(x, mask_c, noise, rnd_normal.reshape(-1).contiguous(), self.P_mean, self.P_std)
        torch.rand(1)                                                      # the cond_p draw of mcedm.py:231 (cond_p = 1: never drops)
        loss = _edm_train_loss(self, x, x_noise, sigma, cond_in, mask_c, None)
        self.log("train_loss", loss, prog_bar=True, on_epoch=True, on_step=False, sync_dist=True)
        return loss

    # ---- sampling -------------------------------------------------------------------------------------
    def sample_edm(self, hu, cond, hu_mask, sparams, return_last=True, guide_dx=False):
        if guide_dx:
            # The reference's own hook for the JOINT model fails: get_dx_pde (models/mcedm.py:500-518) slices the last axis
            # of the NCHW state (`x_denoised[..., 0:h_ch]`) and SweFvLoss then raises "Sizes of tensors must match"
            # (pinned in tests/golden/guided.npz: joint_model_guidance_raises).  Device-side PDE guidance is built where the
            # reference's works: the single-task sampler, mcedm_amd.ddim.PlCondEdm.sample_edm(guide_dx=True).
            raise NotImplementedError("guide_dx=True: the joint model's guidance hook raises in the reference "
                                      "(models/mcedm.py:500-518); use PlCondEdm.sample_edm(guide_dx=True)")
        model = self.ema_model if self.ema_model is not None else self.model
        net = self._net(model)
        n_state = self.h_ch + self.u_ch
        if cond.shape[1] < n_state:
            raise RuntimeError("cond must carry the known state in its first h_ch+u_ch channels (mcedm.py:590)")
        sd = _lib.sampler_desc(sparams, self.sigma_data, self.sigma_min, self.sigma_max)
        hu_noise = torch.randn_like(hu, dtype=torch.float32)
        N, churn = sd.timesteps, self._churns(sd)
        dev_noise = self._noise_mode() == "device" and churn
        step_noise = (torch.randn((N,) + tuple(hu.shape), dtype=torch.float64, device=hu.device)
                      if churn and not dev_noise else None)
        seed = self._draw_seed() if dev_noise else None
        cond, hu_mask, hu_noise = cond.float().contiguous(), hu_mask.float().contiguous(), hu_noise.contiguous()
        with torch.no_grad():
            packed = net.packed_weights()

            def eager(c, m_, i, sn, seed=None):
                return net.plan.sample(packed, sd, c, m_, i, sn, return_last=return_last, ws=self._sample_ws,
                                       rng_seed=self._seed_tensor(seed, i.device))
            kw = dict(seed=seed) if dev_noise else {}
            # the ~4000 launches of one sampling call replay from one HIP graph (lib.GraphedSampler, see _replay)
            B, _, H, W = hu_noise.shape
            key = (B, H, W, bool(return_last), churn, dev_noise, packed.data_ptr(), hu_noise.device.index,
                   _lib.desc_key(sd))
            return self._replay(key, lambda: _lib.GraphedSampler(
                net.plan, packed, sd, B, H, W, masked=True, has_cond=True, churn=churn, return_last=return_last,
                ws=self._sample_ws, device_noise=dev_noise), eager, cond, hu_mask, hu_noise, step_noise, **kw)

    # ---- evaluation loops (host-side bookkeeping, mcedm.py:283-441) ----------------------------------------
    def get_pde_loss(self, x_denoised, x_gt_unnorm=None, noise_level=None, clamp_loss=True, do_rearrange=True,
                     reduce=True):
        if self.pde_loss is None:
            return None
        return self._joint_pde_loss(x_denoised, x_gt_unnorm, noise_level, clamp_loss, do_rearrange, reduce)

    def _unnormalised_mae(self, hu_last, h_unnorm, u_unnorm, mask, loss_dim=None):
        h_un, u_un = self.inverse_data_transform(hu_last[..., 0:self.h_ch], hu_last[..., self.h_ch:self.h_ch + self.u_ch])
        return masked_l1(torch.cat([h_un, u_un], dim=-1), torch.cat([h_unnorm, u_unnorm], dim=-1), mask, loss_dim)

    def validation_step(self, val_batch, batch_idx):
        if (self.current_epoch + 1) % 100 != 0 and self.current_epoch != 0:
            return {"epoch": self.current_epoch}
        h_unnorm, dx, dt, u_unnorm, masks = val_batch
        self.h_ch, self.u_ch = h_unnorm.shape[-1], u_unnorm.shape[-1]
        state_gt = self.data_transform(h_unnorm, u_unnorm)
        noise = torch.randn_like(_nchw(state_gt))
        out = {"epoch": self.current_epoch}
        if self.sparams.type != "edm":
            raise RuntimeError("Non EDM sampler is not supported for the model")
        for name, mask in masks.items():
            cond_in = _nchw(self.get_cond_in(state_gt, mask, dx, dt))
            xs = self.sample_edm(noise, cond_in, _nchw(mask), self.sparams, return_last=True,
                                 guide_dx=self.sparams.guide_dx)
            hu_last = xs[:, -1]
            loss_hu = masked_l1(hu_last, state_gt, mask)
            loss_hu_un = self._unnormalised_mae(hu_last, h_unnorm, u_unnorm, mask)
            self.log(f"val_mae_{name}", loss_hu, prog_bar=True, on_epoch=True, on_step=False, sync_dist=True)
            self.log(f"val_mae_{name}_un", loss_hu_un, prog_bar=True, on_epoch=True, on_step=False, sync_dist=True)
            pde = self.get_pde_loss(hu_last, clamp_loss=False, do_rearrange=False)
            if pde is not None:
                self.log(f"val_pde_loss_{name}", pde / len(h_unnorm), prog_bar=True, on_epoch=True, on_step=False,
                         sync_dist=True)
            out[f"loss_{name}"], out[f"loss_{name}_un"] = loss_hu, loss_hu_un
            out[f"traj_{name}"], out[f"gt_{name}"] = hu_last.unsqueeze(1), state_gt
        return out

    def test_step(self, test_batch, test_idx):
        h_unnorm, dx, dt, u_unnorm, masks = test_batch
        self.h_ch, self.u_ch = h_ch, u_ch = h_unnorm.shape[-1], u_unnorm.shape[-1]
        dm = self.trainer.datamodule
        down_factor = dm.down_factor if dm.down_interp else 1
        state_gt = self.data_transform(h_unnorm, u_unnorm)
        sp = self.test_sparams
        n = sp.n_samples
        state_rep = _nchw(state_gt).repeat(n, 1, 1, 1)
        if sp.type != "edm":
            raise RuntimeError("Non EDM sampler is not supported for the model")
        out = {}
        nb = len(h_unnorm)
        for name, mask in masks.items():
            lo = 0 if name.startswith("h") else h_ch
            loss_dim = torch.arange(lo, lo + (h_ch if name.startswith("h") else u_ch)).long()
            cond_rep = _nchw(self.get_cond_in(state_gt, mask, dx, dt)).repeat(n, 1, 1, 1)
            mask_rep = _nchw(mask).repeat(n, 1, 1, 1)
            noise = torch.randn_like(state_rep)
            xs = self.sample_edm(noise, cond_rep, mask_rep, sp, return_last=sp.return_last, guide_dx=sp.guide_dx)
            xs_mean = xs.reshape(n, nb, *xs.shape[1:]).mean(dim=0)            # '(n b) t h w c -> n b t h w c'
            hu_last = xs_mean[:, -1]
            mask_loss = mask
            if down_factor > 1:
                each = 2 ** (down_factor - 1)
                sel = torch.zeros_like(mask)
                sel[:, ::each, ::each] = 1.0
                mask_loss = mask * sel
            loss_hu = masked_l1(hu_last, state_gt, mask_loss, loss_dim)
            loss_hu_un = self._unnormalised_mae(hu_last, h_unnorm, u_unnorm, mask_loss, loss_dim)
            print(f"\nLoss {name} {loss_hu}, loss {name} un {loss_hu_un}")
            self.log(f"test_mae_{name}", loss_hu, prog_bar=True, on_epoch=True, on_step=False, sync_dist=True)
            self.log(f"test_mae_{name}_un", loss_hu_un, prog_bar=True, on_epoch=True, on_step=False, sync_dist=True)
            pde = self.get_pde_loss(xs[:, -1], clamp_loss=False, do_rearrange=False)
            if pde is not None:
                self.log(f"test_pde_loss_{name}", pde / n / nb, prog_bar=True, on_epoch=True, on_step=False, sync_dist=True)
                pde_gt = self.get_pde_loss(state_gt, clamp_loss=False, do_rearrange=False)
                self.log("test_pde_loss_gt", pde_gt / nb, prog_bar=True, on_epoch=True, on_step=False, sync_dist=True)
            out[f"loss_{name}"], out[f"loss_{name}_un"] = loss_hu, loss_hu_un
            if n < 15:
                last = xs[:, -1]
                # '(n b) h w c -> b h w n c', then a singleton time axis: [b, 1, T, X, n, 2]
                out[f"traj_{name}"] = last.reshape(n, nb, *last.shape[1:]).permute(1, 2, 3, 0, 4).unsqueeze(1)
                out[f"gt_{name}"] = state_gt
        return out
