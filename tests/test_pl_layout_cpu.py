"""CPU: the layout of the four Lightning drop-ins (PlMcedm, PlDdim, PlCondEdm, PlCondDdim) is the one recorded before they
were moved onto the shared base of ``mcedm_amd.pl_base``: state_dict keys in order (tests/golden/pl_layout.npz, names only),
public names and their signatures, plain instance attributes -- and the sharing is by inheritance, not by assigning one class's
functions into another.  The literals below were recorded from the flat classes; they are never generated from the code under
test."""
import inspect

import numpy as np
import pytest

import mcedm_amd  # noqa: F401
from oracle import fixtures as fx
from tests.test_cond_ddim_cpu import ddim_hparams
from tests.test_hip_cond_edm import cond_hparams
from tests.test_hip_ddpm import hparams as ddpm_hparams
from tests.test_hip_eval_steps import _repaint_sampler
from tests.test_hip_module import hparams

SIGNATURES = {'PlCondDdim': {'configure_gradient_clipping': '(self, optimizer, *args, **kwargs)',
                'configure_optimizers': '(self)',
                'data_transform': '(self, h, u)',
                'get_best_by_pde_error': '(self, gt, xs_scaled, n_samples, use_gt=True)',
                'get_cond_in': '(self, h, u, dx, dt)',
                'get_denoised': '(self, model, xt, t, cond=None, x_self_cond=None, dx=None, w=None)',
                'get_edm_steps': '(self)',
                'get_pde_loss': '(self, cond, x_denoised, x_gt_unnorm=None, noise_level=None, clamp_loss=True, '
                                'do_rearrange=True, reduce=True)',
                'get_self_cond_edm': '(self, denoised)',
                'inverse_data_transform': '(self, h, u)',
                'inverse_data_transform_u': '(self, u)',
                'recover_correct_scale': '(self, gt, xs_scaled_mean)',
                'round_sigma': '(self, sigma, return_index=False)',
                'sample': '(self, *a, **k)',
                'sample_edm': '(self, h, u_noise, sparams, return_last=True, guide_dx=False)',
                'scale_back_min_max': '(state_scaled, state_min, state_max)',
                'scale_each_min_max': '(state, return_min_max=False)',
                'set_pde_loss_function': '(self, system, flip_xy)',
                'set_test_sampler_params': '(self, params)',
                'setup': "(self, stage: 'str' = None) -> 'None'",
                'test_step': '(self, test_batch, test_idx)',
                'training_step': '(self, train_batch, batch_idx)',
                'validation_step': '(self, val_batch, batch_idx)'},
 'PlCondEdm': {'configure_optimizers': '(self)',
               'data_transform': '(self, h, u)',
               'get_best_by_pde_error': '(self, gt, xs_scaled, n_samples, use_gt=True)',
               'get_cond_in': '(self, h, u, dx, dt)',
               'get_denoised': '(self, model, xt, t, cond=None, x_self_cond=None, dx=None, w=None)',
               'get_dx_input': '(self, cond, x_denoised)',
               'get_dx_log_prob': '(self, cond, x_denoised, guide_dx)',
               'get_dx_pde': '(self, cond, x_denoised, calc_prob=False)',
               'get_edm_sampler_params': '()',
               'get_loss_weight': '(self, sigma)',
               'get_pde_loss': '(self, cond, x_denoised, x_gt_unnorm=None, noise_level=None, clamp_loss=True, '
                               'do_rearrange=True, reduce=True)',
               'inverse_data_transform': '(self, h, u)',
               'inverse_data_transform_u': '(self, u)',
               'model_precond': '(self, x_noise, sigma, cond=None, x_self_cond=None, dx=None)',
               'recover_correct_scale': '(self, gt, xs_scaled_mean)',
               'sample_edm': '(self, h, u_noise, sparams, return_last=True, guide_dx=False)',
               'scale_back_min_max': '(state_scaled, state_min, state_max)',
               'scale_each_min_max': '(state, return_min_max=False)',
               'set_pde_loss_function': '(self, system, flip_xy)',
               'set_test_sampler_params': '(self, params)',
               'setup': "(self, stage: 'str' = None) -> 'None'",
               'test_step': '(self, test_batch, test_idx)',
               'training_step': '(self, train_batch, batch_idx)',
               'validation_step': '(self, val_batch, batch_idx)'},
 'PlDdim': {'compute_alpha': '(self, t)',
            'data_transform': '(self, h, u)',
            'get_best_by_pde_error': '(self, gt, xs_scaled, n_samples, use_gt=True)',
            'get_denoised': '(self, model, xt, t, cond=None, x_self_cond=None, dx=None, w=None)',
            'get_edm_steps': '(self)',
            'get_pde_loss': '(self, cond, x_denoised, x_gt_unnorm=None, noise_level=None, clamp_loss=True, do_rearrange=True, '
                            'reduce=True)',
            'inverse_data_transform': '(self, h, u)',
            'recover_correct_scale': '(self, gt, xs_scaled_mean)',
            'round_sigma': '(self, sigma, return_index=False)',
            'sample': '(self, *a, **k)',
            'sample_edm': '(self, h, u, sparams, return_last=True, guide_dx=False)',
            'sample_with_repeat': '(self, h, u, sparams, return_last=True, guide_dx=False)',
            'scale_back_min_max': '(state_scaled, state_min, state_max)',
            'scale_each_min_max': '(state, return_min_max=False)',
            'set_pde_loss_function': '(self, system, flip_xy)',
            'set_test_sampler_params': '(self, params)',
            'test_step': '(self, test_batch, test_idx)',
            'training_step': '(self, *a, **k)',
            'validation_step': '(self, val_batch, batch_idx)'},
 'PlMcedm': {'configure_gradient_clipping': '(self, optimizer, *args, **kwargs)',
             'configure_optimizers': '(self)',
             'data_transform': '(self, h, u)',
             'get_cond_in': '(self, x, mask, dx=None, dt=None)',
             'get_denoised': '(self, model, xt, t, cond=None, x_self_cond=None, dx=None, w=None)',
             'get_loss_weight': '(self, sigma)',
             'get_pde_loss': '(self, x_denoised, x_gt_unnorm=None, noise_level=None, clamp_loss=True, do_rearrange=True, '
                             'reduce=True)',
             'get_sampler_params': '(params)',
             'inverse_data_transform': '(self, h, u)',
             'model_precond': '(self, x_noise, sigma, cond=None, x_self_cond=None, dx=None)',
             'round_sigma': '(self, sigma, return_index=False)',
             'sample_edm': '(self, hu, cond, hu_mask, sparams, return_last=True, guide_dx=False)',
             'set_pde_loss_function': '(self, system, flip_xy)',
             'set_test_sampler_params': '(self, params)',
             'setup': "(self, stage: 'str' = None) -> 'None'",
             'test_step': '(self, test_batch, test_idx)',
             'training_step': '(self, train_batch, batch_idx)',
             'validation_step': '(self, val_batch, batch_idx)'}}

ATTRS = {'PlCondDdim': {'_grad_buf': 'None',
                '_stage': 'None',
                '_tables': 'None',
                '_train_generation': '0',
                'amsgrad': 'False',
                'beta1': '0.9',
                'cond_p': '1.0',
                'dx_cond': 'False',
                'dx_detach': 'False',
                'dx_norm': "'l2'",
                'edm_steps': 'None',
                'eps': '1e-08',
                'factor': '0.3',
                'gaussian_dequantization': 'False',
                'h_ch': '1',
                'loss': "'l2'",
                'lr': '0.0002',
                'model_var_type': "'fixedsmall'",
                'node_type': 'False',
                'normalization': "'gauss'",
                'num_timesteps': '1000',
                'optimizer': "'Adam'",
                'pde_loss_lambda': '0.0',
                'rescaled': 'False',
                'sigma_max': 'None',
                'sigma_min': 'None',
                'step_size': '50',
                'u_ch': '1',
                'uniform_dequantization': 'False',
                'weight_decay': '0.0'},
 'PlCondEdm': {'P_mean': '-1.2',
               'P_std': '1.2',
               '_grad_buf': 'None',
               '_train_generation': '0',
               'amsgrad': 'False',
               'beta1': '0.9',
               'cond_p': '1.0',
               'dx_cond': 'False',
               'dx_detach': 'False',
               'dx_norm': "'l2'",
               'eps': '1e-08',
               'gaussian_dequantization': 'False',
               'h_ch': '1',
               'lr': '0.0002',
               'model_var_type': "'fixedsmall'",
               'node_type': 'False',
               'normalization': "'gauss'",
               'num_timesteps': '1000',
               'optimizer': "'Adam'",
               'rescaled': 'False',
               'sigma_data': '1.0',
               'sigma_max': '80',
               'sigma_min': '0.002',
               'u_ch': '1',
               'uniform_dequantization': 'False',
               'weight_decay': '0.0'},
 'PlDdim': {'amsgrad': 'False',
            'beta1': '0.9',
            'cond_p': '0.0',
            'dx_cond': 'False',
            'edm_steps': 'None',
            'eps': '1e-08',
            'gaussian_dequantization': 'False',
            'h_ch': '1',
            'lr': '0.0002',
            'model_var_type': "'fixedsmall'",
            'node_type': 'False',
            'normalization': "'gauss'",
            'num_timesteps': '1000',
            'optimizer': "'Adam'",
            'rescaled': 'False',
            'sigma_max': 'None',
            'sigma_min': 'None',
            'u_ch': '1',
            'uniform_dequantization': 'False',
            'weight_decay': '0.0'},
 'PlMcedm': {'P_mean': '-1.2',
             'P_std': '1.2',
             '_grad_buf': 'None',
             '_train_generation': '0',
             'add_cond_mask': 'False',
             'add_xt': 'False',
             'amsgrad': 'False',
             'beta1': '0.9',
             'cond_p': '1.0',
             'dx_cond': 'False',
             'eps': '1e-08',
             'factor': '0.3',
             'gaussian_dequantization': 'False',
             'h_ch': '1',
             'loss': "'l2'",
             'lr': '0.0002',
             'noise_source': "'device'",
             'normalization': "'gauss'",
             'optimizer': "'Adam'",
             'pde_loss_lambda': '0.0',
             'rescaled': 'False',
             'sigma_data': '1.0',
             'sigma_max': '80',
             'sigma_min': '0.002',
             'step_size': '50',
             'u_ch': '1',
             'uniform_dequantization': 'False',
             'weight_decay': '0.0'}}

NAMES = sorted(SIGNATURES)


@pytest.fixture(scope="module")
def modules():
    from mcedm_amd.ddim import PlCondDdim, PlCondEdm, PlDdim
    from mcedm_amd.mcedm import PlMcedm
    with pytest.MonkeyPatch.context() as mp:
        mp.delenv("MCEDM_NOISE_SOURCE", raising=False)        # the literals were recorded with the constructor's own default
        joint = PlMcedm(hparams(fx.CFG_P))
    return {"PlMcedm": joint,
            "PlCondDdim": PlCondDdim(ddim_hparams()),
            "PlDdim": PlDdim(ddpm_hparams(_repaint_sampler(4, 2, 0.0, 0, 16, 1))),
            "PlCondEdm": PlCondEdm(cond_hparams())}


@pytest.mark.parametrize("name", NAMES)
def test_state_dict_keys_and_their_order(modules, golden, name):
    assert list(modules[name].state_dict().keys()) == [str(k) for k in golden("pl_layout.npz")[name]]


@pytest.mark.parametrize("name", NAMES)
def test_public_names_and_signatures(modules, name):
    cls = type(modules[name])
    for attr, sig in SIGNATURES[name].items():
        assert hasattr(cls, attr), attr
        assert str(inspect.signature(getattr(cls, attr))) == sig, attr


@pytest.mark.parametrize("name", NAMES)
def test_plain_instance_attributes(modules, name):
    got = vars(modules[name])
    for attr, value in ATTRS[name].items():
        assert attr in got and repr(got[attr]) == value, attr


def test_old_import_paths_still_resolve():
    from mcedm_amd import pl_base
    from mcedm_amd.mcedm import DotDict, Normalizer, _Base, _nchw, masked_l1
    for obj in (DotDict, Normalizer, _Base, _nchw, masked_l1):
        assert obj is getattr(pl_base, obj.__name__)


def test_sharing_is_by_inheritance(modules):
    classes = [type(m) for m in modules.values()]
    owners = {}
    for cls in classes:
        for attr, v in vars(cls).items():
            fn = getattr(v, "__func__", v)
            if inspect.isfunction(fn):
                assert fn not in owners, f"{cls.__name__}.{attr} is also {owners[fn]}"
                owners[fn] = f"{cls.__name__}.{attr}"
    edm, ddim = type(modules["PlCondEdm"]), type(modules["PlCondDdim"])
    for attr in ("test_step", "validation_step", "get_cond_in"):
        assert getattr(edm, attr) is getattr(ddim, attr), attr
        assert attr not in vars(edm) and attr not in vars(ddim), attr
