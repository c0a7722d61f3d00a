/* mcedm_hip.h -- C ABI of libmcedm_hip.so, the MI355X (gfx950) implementation of the
 * m-cedm EDM hot path: ADM/EDM U-Net forward (+backward), EDM preconditioning, the
 * deterministic/stochastic Heun sampler, the masked EDM loss and the Adam+EMA step.
 *
 * The reference (katehai/m-cedm) is pure Python and has no FFI of its own; the seam it
 * exposes is Python-level.  Each entry point below names the
 * reference function whose device work it replaces (paths relative to the reference
 * checkout).  INTEGRATION.md shows the ctypes binding a maintainer adds on the
 * reference side.
 *
 * Conventions
 *  - extern "C", plain pointers and sizes only; no torch / C++ types.
 *  - Every entry point returns 0 on success and a negative mcedm_status on failure;
 *    mcedm_last_error() returns a thread-local message for the last failure.
 *  - All device buffers are owned by the caller (parameters, packed weights, workspace,
 *    inputs, outputs).  The library allocates only the host-side plan object.
 *  - Kernels are enqueued on the caller's HIP stream (passed as void* = hipStream_t);
 *    nothing synchronises the device, so calls are graph-capturable.
 *  - Tensors are dense NCHW fp32 unless stated; the sampler state is fp64 like the reference.
 */
#ifndef MCEDM_HIP_H_
#define MCEDM_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MCEDM_ABI_VERSION 4   /* 4: per-plan kernel variants (mcedm_*_plan_set_variant), mcedm_heun_sample_rng;
                               * 3: mcedm_edm_loss / mcedm_sqnorm take caller-owned reduction scratch; mcedm_ddim_timesteps */
/* Device scratch of one grid-wide fixed-order reduction (mcedm_edm_loss, mcedm_sqnorm): 8-byte aligned, contents
 * irrelevant on entry, private to the call until it has completed on its stream.  Two calls that may run concurrently (two
 * plans on two streams of one device) need two scratch areas; calls ordered on one stream can share one. */
#define MCEDM_REDUCE_SCRATCH_BYTES (4096 * 8 + 64)
#define MCEDM_MAX_LEVELS 8

typedef enum {
  MCEDM_OK = 0,
  MCEDM_ERR_INVALID = -1,      /* bad argument / unsupported shape (rejected before any launch) */
  MCEDM_ERR_UNSUPPORTED = -2,  /* configuration outside the hot path (e.g. cond_enc, self_cond) */
  MCEDM_ERR_WORKSPACE = -3,    /* workspace / packed buffer too small */
  MCEDM_ERR_HIP = -4           /* a HIP runtime call or launch failed */
} mcedm_status;

/* Architecture of DhariwalUNet as read from hparams.model (models/adm_blocks.py:203-317,
 * configs/model/adm_edm_mcedm_res32.yaml:4-28).  cat_cond=True, self_cond=False, label_dim=augment_dim=0,
 * dropout=0; dx_cond (network conditioning on the PDE-residual gradient, adm_blocks.py:233-280, 334-362) in both of
 * the reference's forms: dx_mode. */
#define MCEDM_DX_NONE 0   /* dx_cond False */
#define MCEDM_DX_CAT 1    /* dx_cond True, cat_dx True: conv_in reads cat(cond, x, dx) (adm_blocks.py:238, 334-339) */
#define MCEDM_DX_ENC 2    /* dx_cond True, cat_dx False: x_feat = combine_enc(cat(conv_in(.), dx_enc(dx))), dx_enc =
                             Conv3x3 -> GELU -> Conv3x3; dx None -> zero features (adm_blocks.py:266-280, 352-362) */
typedef struct {
  int32_t in_channels;       /* state channels (h_ch + u_ch), 2 */
  int32_t cond_channels;     /* concatenated conditioning channels, 2 (0 = none) */
  int32_t out_channels;      /* out_ch */
  int32_t ch;                /* base width; emb_channels == ch */
  int32_t n_levels;          /* len(ch_mult) */
  int32_t ch_mult[MCEDM_MAX_LEVELS];
  int32_t num_res_blocks;
  int32_t resolution;        /* label only: level names are resolution >> level */
  int32_t n_attn_resolutions;
  int32_t attn_resolutions[MCEDM_MAX_LEVELS];
  int32_t channels_per_head; /* 64 */
  float eps;                 /* GroupNorm eps, 1e-5 */
  int32_t dx_channels;       /* channels of the dx input = hparams.model.in_channels when dx_cond, else 0 */
  int32_t dx_mode;           /* MCEDM_DX_* */
} mcedm_unet_desc;

/* Sampler parameters (configs/diff_sampler/edm_sampler.yaml:1-20; fields read by
 * PlMcedm.sample_edm, models/mcedm.py:570-638). */
typedef struct {
  int32_t timesteps;
  double sigma_min, sigma_max, rho;
  double S_churn, S_min, S_max, S_noise;
  double w;                  /* classifier-free guidance weight; |w| < 1e-3 == off (mcedm.py:453) */
  double sigma_data;         /* 1.0 (mcedm.py:47) */
  double net_sigma_min, net_sigma_max; /* 0.002 / 80 (mcedm.py:49-50) */
} mcedm_sampler_desc;

typedef struct mcedm_plan mcedm_plan;

int mcedm_version(void);
const char* mcedm_last_error(void);

/* ---- plan: the static block list of the network ------------------------------------ */
int mcedm_unet_plan_create(const mcedm_unet_desc* desc, mcedm_plan** out);
void mcedm_unet_plan_destroy(mcedm_plan* plan);

/* Kernel variants of ONE plan (re-entrant per plan).  Every kernel family that exists in two forms is chosen per
 * call in three steps, first hit wins: the plan's own setting (this function; a field of the plan, in force while one of the
 * plan's entry points executes on the calling thread), the process-wide test hooks mcedm_op_set_* below (kernel-level calls
 * have no plan), the environment variable.  value: 1 on, 0 off, -1 back to the process default.  Two plans in one process --
 * on two threads or two streams -- cannot flip each other's kernels.  MCEDM_VARIANT_CONV_WINO also decides how a plan lays
 * out its workspace (whether a block's 1x1 skip projection is folded into conv1): set it before the first
 * mcedm_unet_workspace_bytes / forward of the plan and leave it. */
#define MCEDM_VARIANT_CONV_WINO 0       /* Winograd F(2x2, 3x3) forward / data-gradient convs (env MCEDM_WINOGRAD, default 1) */
#define MCEDM_VARIANT_CONV_WINO1 1      /* its one-wave-per-SIMD form for 128-channel shapes (env MCEDM_WINO1, default 0) */
#define MCEDM_VARIANT_CONV_RESIDENT 2   /* input-resident conv kernels at <= 32 x 32 (env MCEDM_CONV_RESIDENT, default 1) */
#define MCEDM_VARIANT_CONV8 3           /* experimental 8-wave direct conv (env MCEDM_CONV8, default 0) */
#define MCEDM_VARIANT_ATTN_FUSED 4      /* single-launch attention block at 8 x 8 x 64 (env MCEDM_ATTN_FUSED, default 1) */
#define MCEDM_VARIANT_WGRAD_WINO 5      /* Winograd F(3x3, 2x2) weight gradient (env MCEDM_WGRAD_WINO, default 1) */
#define MCEDM_VARIANT_CONV1X1_REG 6     /* register-direct GEMM for un-transformed 1x1 convs at >= 32 x 32 (env MCEDM_CONV1X1_REG, default 1) */
#define MCEDM_VARIANT_CONV_WINO_FOLD 7  /* decoder skip projections computed in the Winograd conv1's epilogue (env MCEDM_WINO_FOLD, default 1); the workspace layout does not depend on it */
#define MCEDM_VARIANT_CONV_WINO_UPZ 8   /* up-sampling Winograd convs skip the positions whose transformed input is exactly zero and stage their input at source resolution (env MCEDM_WINO_UPZ, default 1); bit-identical results, the workspace layout does not depend on it */
#define MCEDM_VARIANT_CONV_WINO_SPLIT 9 /* 3x3 convs below 32 x 32 on the Winograd kernel with the positions split over the waves (env MCEDM_WINO_SPLIT, default 1); the workspace layout does not depend on it */
int mcedm_unet_plan_set_variant(mcedm_plan* plan, int which, int value);

/* Dropout of the ADM U-Net's training step (models/adm_blocks.py:170: conv1 reads F.dropout(silu(film(norm1(h))), p, training)).
 * A setting of the plan, honoured by every training entry -- mcedm_unet_forward[_dx] and mcedm_edm_denoise[_dx] with
 * training != 0, and every backward entry -- and ignored by training = 0 calls and by every sampler.  0 <= p < 1; p = 0 is "off"
 * (the state of a new plan; rng_seed is then not kept); p >= 1, negative or NaN, and p > 0 with rng_seed NULL, are
 * MCEDM_ERR_INVALID.  rng_seed: DEVICE memory, one 64-bit seed, read by the kernels when the forward runs (like every `_rng`
 * entry's); the forward copies the value it used into the workspace, on the stream, and the backward regenerates its masks from
 * that copy, so the host may rewrite *rng_seed between the two.
 * The mask contract.  Block j is the 0-based position of a block in the order the network runs them (encoder blocks, then decoder
 * blocks); its mask covers conv1's input [B, cout, H, W].  With u = what mcedm_uniform_fill(u, B * cout * H * W, rng_seed,
 * draw = j) writes, element e = ((b * cout + c) * H + y) * W + x is KEPT iff u[e] >= (float)p; a kept value is multiplied by
 * 1.0f / (1.0f - (float)p) in fp32, a dropped value is exactly 0.0f (also where the activation is NaN or Inf: torch multiplies by
 * zero there and keeps the NaN).  The kernels generate u in registers, one Philox block per four consecutive elements, and never
 * read a mask tensor.  The training workspace grows by one conv1-input-sized tensor per block (256-byte aligned) and a 256-byte
 * seed slot while p > 0: mcedm_unet_workspace_bytes(training = 1) reports it; at p = 0, and for training = 0 at any p, every size
 * is what it was. */
int mcedm_unet_plan_set_dropout(mcedm_plan* plan, double p, const uint64_t* rng_seed);

/* Parameter table in DhariwalUNet.state_dict() order (parameters only, no buffers).
 * name is owned by the plan. */
int mcedm_unet_param_count(const mcedm_plan* plan);
int mcedm_unet_param_info(const mcedm_plan* plan, int index, const char** name, int64_t* numel,
                          int32_t* ndim, int64_t shape[4]);

/* Derived ("packed") weights: MFMA-friendly copies of the conv / linear weights.  Must be
 * re-run whenever a parameter changes.  params[i] is the device pointer of parameter i. */
int mcedm_unet_packed_bytes(const mcedm_plan* plan, size_t* bytes);
int mcedm_unet_pack_weights(const mcedm_plan* plan, const float* const* params, void* packed, void* stream);

/* Workspace needed by one forward at batch B and spatial size HxW (H, W multiples of
 * 2^(n_levels-1)).  training != 0 keeps every activation the backward needs. */
int mcedm_unet_workspace_bytes(const mcedm_plan* plan, int B, int H, int W, int training, size_t* bytes);

/* DhariwalUNet.forward (models/adm_blocks.py:364-404): out = F(cat(cond, x_scale * x), noise_labels).
 *  x            [B, in_channels, H, W]
 *  cond         [B, cond_channels, H, W] or NULL (treated as zeros, adm_blocks.py:328-331)
 *  x_scale      [n_noise] per-sample factor applied to x while it is read (EDM c_in), or NULL (= 1)
 *  noise_labels [n_noise], n_noise == 1 (broadcast, sampling) or == B (training)
 *  out          [B, out_channels, H, W] */
int mcedm_unet_forward(const mcedm_plan* plan, const void* packed, const float* x, const float* cond,
                       const float* x_scale, const float* noise_labels, int n_noise, float* out,
                       void* workspace, size_t workspace_bytes, int B, int H, int W, int training,
                       void* stream);

/* PlMcedm.model_precond / get_denoised with w == 0 (models/mcedm.py:199-211, 443-461):
 * D = c_skip*x + c_out*F(c_in*x, ln(sigma)/4, cond).  sigma is a device array of n_sigma (1 or B)
 * fp32 values.  F_out may be NULL. */
int mcedm_edm_denoise(const mcedm_plan* plan, const void* packed, const float* x, const float* sigma,
                      int n_sigma, const float* cond, float* D_out, float* F_out, void* workspace,
                      size_t workspace_bytes, int B, int H, int W, int training, double sigma_data,
                      void* stream);

/* PlMcedm.sample_edm (models/mcedm.py:570-638), guide_dx False / dx_cond False.
 *  cond       [B, cond_channels, H, W] fp32; its first in_channels channels are hu_known
 *  mask       [B, in_channels, H, W] fp32, 1 = missing; NULL = no mask: the unmasked single-task sampler of
 *             PlCondEdm.sample_edm (models/ddim.py:1532-1601), where cond is pure conditioning (may be NULL)
 *  init_noise [B, in_channels, H, W] fp32  (the reference's randn_like(hu), mcedm.py:576)
 *  step_noise [timesteps, B, in_channels, H, W] fp64 or NULL (the per-step randn_like(x_cur) of
 *             mcedm.py:608, fp64 like x_cur; NULL is only legal when no step has gamma > 0)
 *  out        fp64, [B, 1, H, W, C] if return_last else [B, timesteps+1, H, W, C]
 *  workspace must hold mcedm_sampler_workspace_bytes(). */
int mcedm_sampler_workspace_bytes(const mcedm_plan* plan, int B, int H, int W, size_t* bytes);
int mcedm_heun_sample(const mcedm_plan* plan, const void* packed, const mcedm_sampler_desc* sp,
                      const float* cond, const float* mask, const float* init_noise,
                      const double* step_noise, double* out, int return_last, void* workspace,
                      size_t workspace_bytes, int B, int H, int W, void* stream);

/* mcedm_heun_sample with the per-step churn noise drawn ON THE DEVICE: models/mcedm.py:604-608 draws randn_like(x_cur) in every
 * step; here the kernel that applies `x_hat = x_cur + sqrt(t_hat^2 - t_cur^2) * S_noise * eps * mask` generates eps itself
 * (Philox4x32-10 + Box-Muller in fp64; key = the 64-bit seed at *rng_seed in DEVICE memory, counter = (element pair, step index)),
 * so there is no [timesteps][B][C][H][W] fp64 step_noise tensor and a captured HIP graph replays with fresh noise once the host
 * has written a new seed.  Same moments as, but not the stream of, torch's generator; mcedm_normal_fill(out, n, rng_seed, draw = i)
 * writes step i's draw out, and feeding those tensors to mcedm_heun_sample reproduces this call bit for bit. */
int mcedm_heun_sample_rng(const mcedm_plan* plan, const void* packed, const mcedm_sampler_desc* sp, const float* cond,
                          const float* mask, const float* init_noise, const uint64_t* rng_seed, double* out, int return_last,
                          void* workspace, size_t workspace_bytes, int B, int H, int W, void* stream);
/* PDE guidance inside the single-task sampler (PlCondEdm.sample_edm with guide_dx=True, models/ddim.py:1532-1601:
 * get_dx_log_prob :641-650 -> get_dx_pde :1424-1450, used at :1577-1579 and :1589-1591): after every denoiser call
 * dx = mean over the two fields of d residual(x_unnorm) / d x_unnorm, x_unnorm = (h from cond[:, 0], u = denoised state),
 * and d = (x - D) / t - weight * dx / t_hat.  system 1 = SweFvLoss (FORCE finite-volume residual along W), system 2 =
 * DarcyLoss in its log-probability form (calc_prob=True).  sub_* / div_* are the normalisers' statistics (scalars):
 * x_unnorm = x * div + sub.  mask must be NULL, in_channels 1, cond_channels >= 1.  (The joint model's hook,
 * models/mcedm.py:500-518, slices the wrong axis and raises in the reference; it is not built.) */
typedef struct {
  int32_t system;
  float half_dt, dx;         /* SWE: (float)(0.5 * Tn / n_times) and x[1] - x[0] of SweFvLoss.gen_x (fp32), as for mcedm_swe_fv_residual */
  float two_dx;              /* Darcy: (float)(2 * D / s), as for mcedm_darcy_residual */
  float sub_h, div_h, sub_u, div_u;
  double weight;             /* 5.0 (mcedm.py:616) */
} mcedm_guidance_desc;
int mcedm_heun_sample_guided(const mcedm_plan* plan, const void* packed, const mcedm_sampler_desc* sp,
                             const mcedm_guidance_desc* gd, const float* cond, const float* mask,
                             const float* init_noise, const double* step_noise, double* out, int return_last,
                             void* workspace, size_t workspace_bytes, int B, int H, int W, void* stream);
/* mcedm_heun_sample_guided with rng_seed in place of step_noise: the churn draws are generated on the device exactly as in
 * mcedm_heun_sample_rng (draw index = step index; mcedm_normal_fill's tensors fed to mcedm_heun_sample_guided reproduce the call
 * bit for bit).  A NULL rng_seed is MCEDM_ERR_INVALID; every other check is mcedm_heun_sample_guided's. */
int mcedm_heun_sample_guided_rng(const mcedm_plan* plan, const void* packed, const mcedm_sampler_desc* sp,
                                 const mcedm_guidance_desc* gd, const float* cond, const float* mask, const float* init_noise,
                                 const uint64_t* rng_seed, double* out, int return_last, void* workspace, size_t workspace_bytes,
                                 int B, int H, int W, void* stream);
/* ---- dx_cond: the network conditioned on the PDE-residual gradient (plans with dx_mode != MCEDM_DX_NONE) ----------
 * The same three calls with the extra network input dx [B, dx_channels, H, W] (DhariwalUNet.forward(..., dx=dx),
 * adm_blocks.py:364-388; model_precond / get_denoised with dx, models/ddim.py:1661-1666, 1745-1763).  dx == NULL is the
 * reference's dx=None: zeros concatenated (cat_dx) or zero dx features (dx_enc).  The entry points without _dx accept such
 * plans too and mean dx = NULL.  dx carries no gradient (torch.autograd.grad without create_graph, models/pde_loss.py:233;
 * dx_detach); the backward returns the gradients of dx_enc / combine_enc like every other parameter.  n_buckets == 0: no
 * bucket events. */
int mcedm_unet_forward_dx(const mcedm_plan* plan, const void* packed, const float* x, const float* dx, const float* cond,
                          const float* x_scale, const float* noise_labels, int n_noise, float* out, void* workspace,
                          size_t workspace_bytes, int B, int H, int W, int training, void* stream);
int mcedm_edm_denoise_dx(const mcedm_plan* plan, const void* packed, const float* x, const float* dx, const float* sigma,
                         int n_sigma, const float* cond, float* D_out, float* F_out, void* workspace,
                         size_t workspace_bytes, int B, int H, int W, int training, double sigma_data, void* stream);
int mcedm_edm_denoise_backward_dx(const mcedm_plan* plan, const void* packed, const float* const* params, const float* x,
                                  const float* dx, const float* sigma, int n_sigma, const float* cond, const float* dD,
                                  float* const* grads, void* workspace, size_t workspace_bytes, int B, int H, int W,
                                  double sigma_data, int n_buckets, const int32_t* bucket_first_param,
                                  void* const* bucket_events, void* stream);
/* PlCondEdm.sample_edm of a dx_cond model (models/ddim.py:1532-1601): before EVERY denoiser call
 * dx_in = get_dx_input(h, x) (:601-639 with dx_norm == 'prob', the only normalisation the single-task get_dx_pde :1424-1450
 * can feed: its calc_prob=False result is 3-D and the other branches fail to unpack it) = the mean over the two fields of
 * the log-probability residual gradient at x_unnorm = (h from cond[:, 0], u = the CURRENT NOISY state cast to fp32), fed to
 * the network as dx.  dxc describes that residual (same fields as for mcedm_heun_sample_guided; weight unused); gd != NULL
 * additionally applies guide_dx to the denoised state as in mcedm_heun_sample_guided.  With sp->w != 0 the unconditional
 * branch runs without cond AND without dx (:1759-1760). */
int mcedm_heun_sample_dxcond(const mcedm_plan* plan, const void* packed, const mcedm_sampler_desc* sp,
                             const mcedm_guidance_desc* dxc, const mcedm_guidance_desc* gd, const float* cond,
                             const float* init_noise, const double* step_noise, double* out, int return_last,
                             void* workspace, size_t workspace_bytes, int B, int H, int W, void* stream);
/* The same with rng_seed in place of step_noise (draw index = step index, as in mcedm_heun_sample_rng). */
int mcedm_heun_sample_dxcond_rng(const mcedm_plan* plan, const void* packed, const mcedm_sampler_desc* sp,
                                 const mcedm_guidance_desc* dxc, const mcedm_guidance_desc* gd, const float* cond,
                                 const float* init_noise, const uint64_t* rng_seed, double* out, int return_last, void* workspace,
                                 size_t workspace_bytes, int B, int H, int W, void* stream);
/* Host helper: the float64 sigma schedule of mcedm.py:584-588 (timesteps+1 values, last = 0). */
int mcedm_edm_t_steps(const mcedm_sampler_desc* sp, double* t_steps);

/* ---- training --------------------------------------------------------------------- */
/* Masked, weighted EDM loss of training_step (models/mcedm.py:266-278, models/losses.py:48-59)
 * and its gradient w.r.t. D:  loss = mean_b sum_chw w_b (D*m - x*m)^2,  w_b = (s^2+sd^2)/(s*sd)^2.
 *  loss_out: 1 fp32 (device), accumulated from zero by this call;  dD_out [B,C,H,W] or NULL.
 *  mask == NULL: unmasked loss of PlCondEdm.training_step (models/ddim.py:1727).
 *  scratch: MCEDM_REDUCE_SCRATCH_BYTES of device memory (the per-block partial sums and the ticket of the fixed-order,
 *  atomic-free sum that makes the loss bitwise reproducible): the library keeps no device state of its own. */
int mcedm_edm_loss(const float* D, const float* x, const float* mask, const float* sigma, int B, int C,
                   int H, int W, double sigma_data, float* loss_out, float* dD_out, void* scratch, size_t scratch_bytes,
                   void* stream);

/* x_noise = x + mask*noise*sigma (mcedm.py:216; mask == NULL: x + noise*sigma, :218), sigma = exp(rnd_normal*P_std + P_mean)
 * (mcedm.py:271). */
int mcedm_edm_noise_inputs(const float* x, const float* mask, const float* noise, const float* rnd_normal,
                           int B, int C, int H, int W, double P_mean, double P_std, float* x_noise,
                           float* sigma_out, void* stream);

/* Backward of mcedm_edm_denoise through the U-Net: consumes the activations kept in
 * `workspace` by the matching forward (training != 0).  grads[i] receives dLoss/dparam_i
 * (overwritten).  dD is the gradient w.r.t. D_out. */
int mcedm_edm_denoise_backward(const mcedm_plan* plan, const void* packed, const float* const* params,
                               const float* x, const float* sigma, int n_sigma, const float* cond,
                               const float* dD, float* const* grads, void* workspace,
                               size_t workspace_bytes, int B, int H, int W, double sigma_data, void* stream);

/* Overlap hook for the data-parallel gradient exchange (the DDP bucketed all-reduce behind
 * configs/trainer/trainer_ddim.yaml:7 `strategy: ddp`).  Same as
 * mcedm_edm_denoise_backward, and additionally records the caller's HIP events on `stream`: bucket_events[k]
 * (hipEvent_t) is recorded as soon as the gradient of EVERY parameter with index >= bucket_first_param[k] has been
 * enqueued.  The backward finishes parameters from the last (out_conv) to the first (map_layer0), so the caller can
 * all-reduce bucket k = parameters [bucket_first_param[k], bucket_first_param[k-1]) on another stream (after
 * hipStreamWaitEvent) while the rest of the backward still runs.  bucket_first_param must decrease, end with 0 and
 * name first parameters of blocks; mcedm_unet_grad_buckets proposes such a split into at most max_buckets
 * roughly equal parts.  The library itself stays free of any communication dependency: the collective is the
 * caller's (RCCL through torch.distributed in m-cedm_amd/train.py). */
int mcedm_unet_grad_buckets(const mcedm_plan* plan, int max_buckets, int32_t* first_param, int* n_buckets);
int mcedm_edm_denoise_backward_bucketed(const mcedm_plan* plan, const void* packed, const float* const* params,
                                        const float* x, const float* sigma, int n_sigma, const float* cond,
                                        const float* dD, float* const* grads, void* workspace,
                                        size_t workspace_bytes, int B, int H, int W, double sigma_data,
                                        int n_buckets, const int32_t* bucket_first_param,
                                        void* const* bucket_events, void* stream);

/* Squared L2 norm of a flat fp32 buffer, accumulated in fp64 into *sqnorm_out (device, overwritten); fixed summation
 * order (bitwise reproducible).  scratch: MCEDM_REDUCE_SCRATCH_BYTES of device memory, as for mcedm_edm_loss. */
int mcedm_sqnorm(const float* g, size_t n, double* sqnorm_out, void* scratch, size_t scratch_bytes, void* stream);

/* Fused grad-clip + Adam + EMA on flat fp32 buffers (models/mcedm.py:139-168,
 * models/ddim_blocks.py:44-54, configs/trainer/trainer_ddim.yaml:8-9).
 *  clip = min(1, max_norm / (sqrt(*sqnorm) + 1e-6)) is computed on device from sqnorm (NULL = no clip);
 *  grad_scale multiplies grads first (1/world_size after a sum all-reduce). `step` counts from 1. */
int mcedm_adam_ema_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float* ema,
                        size_t n, double lr, double beta1, double beta2, double eps, double weight_decay,
                        const double* sqnorm, double max_norm, double grad_scale, double ema_beta,
                        int64_t step, void* stream);

/* ---- epsilon-prediction (DDPM) training and VP sampling of the ADM U-Net: PlCondDdim, models/ddim.py:1053-1605 ----------
 * Self-conditioning (hparams.model.self_cond, adm_blocks.py:227-238, 318-338) needs no plan of its own: conv_in reads
 * cat(cond, x_self_cond, x), which is the cat_cond network with cond_channels' = cond_channels + in_channels fed
 * cond' = cat(cond or 0, x_self_cond or 0) -- the same parameter table, conv_in's weight [ch, cond + 2 in, 3, 3] included.
 * The entries below write cond' into a caller buffer [B, cond_channels + in_channels, H, W] instead of a torch.cat. */

/* x_noise = x * sqrt_ab[t_b] + noise * sqrt_1mab[t_b] and labels[b] = (float)t_b  (PlDdim.forward, models/ddim.py:195-197;
 * the labels are t.float(), :206, 209).  sqrt_ab / sqrt_1mab: n_table fp32 values on the device, (1 - betas).cumprod(0).sqrt()
 * and (1 - that).sqrt() formed by the caller with the reference's expression; t: B int64 device values in [0, n_table). */
int mcedm_eps_noise_inputs(const float* x, const float* noise, const int64_t* t, const float* sqrt_ab, const float* sqrt_1mab,
                           int n_table, int B, int C, int H, int W, float* x_noise, float* labels, void* stream);
/* Self-conditioning input cond' [B, cond_channels + in_channels, H, W]: channels [0, cond_channels) = cond (NULL: zeros, the
 * conditioning switched off, models/ddim.py:202-203), channels [cond_channels, +in_channels) = the self-conditioning estimate
 * x_sc = (x_noise - F0 * sqrt_1mab[t_b]) / sqrt_ab[t_b] of the no-grad pre-pass F0 = model(x_noise, t, cond)
 * (models/ddim.py:205-210); F0 == NULL: zeros (no pre-pass this batch; x_noise, t and the tables may then be NULL too). */
int mcedm_eps_self_cond(const float* x_noise, const float* F0, const int64_t* t, const float* sqrt_ab, const float* sqrt_1mab,
                        int n_table, const float* cond, int cond_channels, int in_channels, int B, int H, int W,
                        float* cond_out, void* stream);
/* NoiseEstimationLoss (models/losses.py:39-59): loss = mean_b sum_chw (F - eps)^2 and dF = 2 (F - eps) / B (NULL: not written).
 * loss_out: 1 fp32 (device).  scratch as for mcedm_edm_loss: the same fixed-order, atomic-free sum (bitwise reproducible). */
int mcedm_eps_loss(const float* F, const float* eps, int B, int C, int H, int W, float* loss_out, float* dF_out, void* scratch,
                   size_t scratch_bytes, void* stream);
/* Backward of mcedm_unet_forward(..., training = 1) through the U-Net from dF = dLoss/d out (the EDM entries start from dD and
 * scale it by c_out first).  x, cond, x_scale, noise_labels, n_noise: the arguments of that forward, whose activations
 * `workspace` still holds (mcedm_unet_workspace_bytes(training = 1)).  grads[i] receives dLoss/dparam_i (overwritten).  The
 * _bucketed form records bucket_events as mcedm_edm_denoise_backward_bucketed does. */
int mcedm_unet_backward(const mcedm_plan* plan, const void* packed, const float* const* params, const float* x,
                        const float* cond, const float* x_scale, const float* noise_labels, int n_noise, const float* dF,
                        float* const* grads, void* workspace, size_t workspace_bytes, int B, int H, int W, void* stream);
int mcedm_unet_backward_bucketed(const mcedm_plan* plan, const void* packed, const float* const* params, const float* x,
                                 const float* cond, const float* x_scale, const float* noise_labels, int n_noise,
                                 const float* dF, float* const* grads, void* workspace, size_t workspace_bytes, int B, int H,
                                 int W, int n_buckets, const int32_t* bucket_first_param, void* const* bucket_events,
                                 void* stream);
/* mcedm_unet_backward_bucketed for a dx_cond plan, after mcedm_unet_forward_dx(..., training = 1): dx [B, dx_channels, H, W] is
 * that forward's (NULL: None -- the gradients of dx_enc.* are then exactly zero, those of combine_enc.* are not).  n_buckets == 0
 * records no events, as in mcedm_edm_denoise_backward_dx.  The two entries above keep refusing dx_cond plans. */
int mcedm_unet_backward_dx(const mcedm_plan* plan, const void* packed, const float* const* params, const float* x,
                           const float* dx, const float* cond, const float* x_scale, const float* noise_labels, int n_noise,
                           const float* dF, float* const* grads, void* workspace, size_t workspace_bytes, int B, int H, int W,
                           int n_buckets, const int32_t* bucket_first_param, void* const* bucket_events, void* stream);

/* VP-preconditioned Heun sampler of an epsilon network (PlCondDdim.sample_edm, models/ddim.py:1532-1601, around get_denoised
 * :915-947): D = x + (-sigma) F(c_in x, c_noise, c_in cond), c_in = 1 / sqrt(sigma^2 + 1) in fp32, state fp64.  The host
 * rounds the schedule onto edm_steps (round_sigma, :949-957) and passes the result; the evaluation at t_hat[i] uses
 * c_noise[2 i], the correction at t_steps[i + 1] c_noise[2 i + 1] (the last step has none).  cond carries the first
 * cond_channels channels of the plan's conditioning input; the rest (self-conditioning, get_self_cond_edm returns None,
 * :1603-1605) read zeros.  |w| >= 1e-3 with cond given: F = (w + 1) F(cond) - w F(no cond) (:941-942).  All host arrays are
 * read during the call only. */
typedef struct {
  int32_t timesteps;         /* N */
  int32_t cond_channels;     /* channels of `cond`; <= the plan's cond_channels */
  const double* t_steps;     /* N + 1 host values, rounded, t_steps[N] = 0 */
  const double* t_hat;       /* N host values, round_sigma(t_cur + gamma t_cur) */
  const float* c_noise;      /* 2 N host values, num_timesteps - 1 - index(round_sigma(sigma)) */
  double S_noise;
  double w;
} mcedm_vp_sampler_desc;
int mcedm_vp_sampler_workspace_bytes(const mcedm_plan* plan, int B, int H, int W, size_t* bytes);
/* init_noise [B, in, H, W] fp32 (x_0 = init_noise * t_steps[0] in fp64); step_noise [N, B, in, H, W] fp64, step i's
 * randn_like(x_cur) (NULL only when t_hat[i] == t_steps[i] for every i); out fp64 [B, 1 or N + 1, H, W, in]. */
int mcedm_vp_heun_sample(const mcedm_plan* plan, const void* packed, const mcedm_vp_sampler_desc* sp, const float* cond,
                         const float* init_noise, const double* step_noise, double* out, int return_last, void* workspace,
                         size_t workspace_bytes, int B, int H, int W, void* stream);
/* The same with the churn noise generated on the device, as mcedm_heun_sample_rng does (draw = step index). */
int mcedm_vp_heun_sample_rng(const mcedm_plan* plan, const void* packed, const mcedm_vp_sampler_desc* sp, const float* cond,
                             const float* init_noise, const uint64_t* rng_seed, double* out, int return_last, void* workspace,
                             size_t workspace_bytes, int B, int H, int W, void* stream);
/* mcedm_vp_heun_sample / _rng in one signature (at most one of step_noise and rng_seed non-NULL, else MCEDM_ERR_INVALID) with
 * PDE guidance (guide_dx=True): after each get_denoised, dx = get_dx_log_prob(h, D) on the fp32 D (models/ddim.py:1576, 1589 ->
 * get_dx_pde :1424-1450; h = cond[:, 0] of the caller's unscaled cond, u = D) and
 *   d_cur = (x_hat - D) / t_hat - weight * dx / t_hat,  d_prime = (x_next - D') / t_next - weight * dx' / t_hat   (:1576-1578, 1589-1590)
 * -- both stages divide by t_hat.  gd: the description of mcedm_heun_sample_guided, weight 5.0 in the reference.  gd == NULL
 * reproduces the unguided entry bit for bit.  gd != NULL requires in_channels == 1, cond != NULL, sp->cond_channels >= 1,
 * gd->system in {1, 2} and, for Darcy, a square grid larger than 4 x 4: otherwise MCEDM_ERR_INVALID before any launch.  The workspace
 * (mcedm_vp_guided_workspace_bytes) is the unguided one plus the gradient [B, 1, H, W] and the Darcy scratch; with gd == NULL the
 * unguided size suffices. */
int mcedm_vp_guided_workspace_bytes(const mcedm_plan* plan, int B, int H, int W, size_t* bytes);
int mcedm_vp_heun_sample_guided(const mcedm_plan* plan, const void* packed, const mcedm_vp_sampler_desc* sp,
                                const mcedm_guidance_desc* gd, const float* cond, const float* init_noise, const double* step_noise,
                                const uint64_t* rng_seed, double* out, int return_last, void* workspace, size_t workspace_bytes,
                                int B, int H, int W, void* stream);
/* PlCondDdim.sample_edm of a dx_cond model (hparams.model.dx_cond with dx_norm 'prob'): mcedm_vp_heun_sample_guided's signature
 * with dxc in front of gd.  In front of EACH of the two get_denoised calls of a step, dx_in = get_dx_input(h, x) (:1571, 1584 ->
 * get_dx_pde :1424-1450 with calc_prob: the mean of the two field gradients, [B, 1, H, W]) at the current state x cast to fp32
 * (x_hat, then the Euler x_next), h = cond[:, 0] of the caller's unscaled cond; the network reads fl(c_in * dx_in) (:933-934:
 * here dx IS scaled, unlike mcedm_heun_sample_dxcond) -- one fp32 rounding of the finished mean, formed where the gradient
 * kernel stores it.  With |sp->w| >= 0.001 the second evaluation reads neither cond nor dx (:938-942).  dxc: the description of
 * mcedm_heun_sample_dxcond (weight unused); gd: PDE guidance on top, NULL = none, with a gradient buffer of its own.  Before any
 * launch, MCEDM_ERR_INVALID unless: the plan has dx_mode != MCEDM_DX_NONE, in_channels == 1 and dx_channels == 1; dxc != NULL with
 * system 1 or 2; cond != NULL with sp->cond_channels >= 1; for Darcy H == W > 4; gd passes mcedm_vp_heun_sample_guided's checks;
 * at most one of step_noise and rng_seed is given.  mcedm_vp_dxcond_workspace_bytes sizes the call with dxc AND gd (exact);
 * without gd one gradient buffer less is needed.  There is no _rng twin.  mcedm_vp_heun_sample[_rng|_guided] keep refusing dx_cond
 * plans. */
int mcedm_vp_dxcond_workspace_bytes(const mcedm_plan* plan, int B, int H, int W, size_t* bytes);
int mcedm_vp_heun_sample_dxcond(const mcedm_plan* plan, const void* packed, const mcedm_vp_sampler_desc* sp,
                                const mcedm_guidance_desc* dxc, const mcedm_guidance_desc* gd, const float* cond,
                                const float* init_noise, const double* step_noise, const uint64_t* rng_seed, double* out,
                                int return_last, void* workspace, size_t workspace_bytes, int B, int H, int W, void* stream);

/* PlCondDdim.sample (models/ddim.py:1452-1530): the DDIM sampler of the single-task conditional network, guide_dx False,
 * dx_cond False.  Everything is fp32 like the reference; one network evaluation per step, two with guidance, and one fused
 * elementwise kernel per step.
 *  timesteps, skip_type (0 uniform, 1 quad), eta, alphas_cumprod_ext, num_diffusion_timesteps: as in mcedm_ddim_desc; the
 *                  sequence walked is mcedm_ddim_timesteps', last entry first, S entries (uniform: S may exceed timesteps)
 *  w               classifier-free guidance: |w| >= 0.001 adds a second pass whose cond channels read zeros,
 *                  et = (w + 1) F(cond) - w F(None) (:1493-1497)
 *  cond_channels   channels of `cond`; the plan's conditioning input is cat(cond, x_self_cond)
 *  self_cond       1: the previous step's x0 prediction is fed back as x_self_cond (zeros in the first step, :1490), which
 *                  needs a plan with cond_channels + in_channels conditioning channels; 0: those channels stay zero
 *  cond            [B, cond_channels, H, W] (NULL iff cond_channels == 0);  init_noise [B, in, H, W]
 *  eta_noise       [S, B, in, H, W]: step k's torch.rand_like draw of :1512 (UNIFORM in the reference) in slice k, in the order
 *                  the steps are walked; required exactly when |eta| > 1e-10, else ignored and may be NULL
 *  xs_out, x0_out  fp32 'b t h w c': [B, S + 1, H, W, in] with init_noise in slot 0 and [B, S, H, W, in]; one slot each with
 *                  return_last (the last state and the last x0 prediction)
 * The workspace holds xt, xt_next, F, F_uncond, cond' and its zero-cond twin in front of the network's own workspace. */
typedef struct mcedm_cond_ddim_desc {
  int32_t timesteps, skip_type;
  double eta, w;
  int32_t cond_channels, self_cond, num_diffusion_timesteps;
  const float* alphas_cumprod_ext;
} mcedm_cond_ddim_desc;
int mcedm_cond_ddim_workspace_bytes(const mcedm_plan* plan, int B, int H, int W, size_t* bytes);
int mcedm_cond_ddim_sample(const mcedm_plan* plan, const void* packed, const mcedm_cond_ddim_desc* sp, const float* cond,
                           const float* init_noise, const float* eta_noise, float* xs_out, float* x0_out, int return_last,
                           void* workspace, size_t workspace_bytes, int B, int H, int W, void* stream);
/* mcedm_cond_ddim_sample with rng_seed in place of eta_noise: the fused step kernel generates the uniform draw of step k (in the
 * order the steps are walked) itself, as draw k of the uniform generator below (mcedm_uniform_fill) keyed by the 64-bit seed at
 * *rng_seed in DEVICE memory, read when the kernel runs -- one Philox block per 16-byte group in registers instead of a 16-byte
 * load, no [S, B, in, H, W] tensor, and a captured HIP graph replays with fresh noise once the host has rewritten the seed.
 * Bit-for-bit contract: mcedm_uniform_fill(slice k of eta_noise, B * in * H * W, rng_seed, k) for every k, handed to
 * mcedm_cond_ddim_sample, reproduces this call.  With |eta| <= 1e-10 the seed is never read.  A NULL rng_seed is
 * MCEDM_ERR_INVALID; every other check is mcedm_cond_ddim_sample's. */
int mcedm_cond_ddim_sample_rng(const mcedm_plan* plan, const void* packed, const mcedm_cond_ddim_desc* sp, const float* cond,
                               const float* init_noise, const uint64_t* rng_seed, float* xs_out, float* x0_out, int return_last,
                               void* workspace, size_t workspace_bytes, int B, int H, int W, void* stream);
/* mcedm_cond_ddim_sample / _rng in one signature (at most one of eta_noise and rng_seed non-NULL, else MCEDM_ERR_INVALID) with PDE
 * guidance (guide_dx=True, models/ddim.py:1499-1503): per step, after the classifier-free blend of et,
 *   dx = get_dx_log_prob(h, xt)  at the CURRENT NOISY STATE xt (:1501; h = cond[:, 0], u = xt, get_dx_pde :1424-1450)
 *   et = et - weight * (1 - at).sqrt() * dx                                                                  (:1502-1503)
 * in fp32 in that order (gw = fl(weight * s1), g = fl(gw * dx), et = fl(et - g)); the guided et feeds x0_t, the next step's
 * x_self_cond and xt_next (:1505-1515).  The guidance launches of a step go in front of its network launches.  gd, its checks, the
 * gd == NULL case and the workspace (mcedm_cond_ddim_guided_workspace_bytes): as for mcedm_vp_heun_sample_guided. */
int mcedm_cond_ddim_guided_workspace_bytes(const mcedm_plan* plan, int B, int H, int W, size_t* bytes);
int mcedm_cond_ddim_sample_guided(const mcedm_plan* plan, const void* packed, const mcedm_cond_ddim_desc* sp,
                                  const mcedm_guidance_desc* gd, const float* cond, const float* init_noise, const float* eta_noise,
                                  const uint64_t* rng_seed, float* xs_out, float* x0_out, int return_last, void* workspace,
                                  size_t workspace_bytes, int B, int H, int W, void* stream);
/* PlCondDdim.sample of a dx_cond model: mcedm_cond_ddim_sample_guided's signature with dxc in front of gd.  At every step
 * dx_in = get_dx_input(h, xt) (:1492) at the step's CURRENT noisy state xt (the first step's is init_noise), UNSCALED, is the dx
 * input of model(xt, t, cond=h, x_self_cond, dx=dx_in); its launches go in front of the step's network launches.  With
 * |sp->w| >= 0.001 the second pass keeps the self-conditioning channels and reads neither cond nor dx (:1495-1497).  The first
 * step has dx but no x_self_cond.  dxc, gd, the checks, the missing _rng twin and the workspace
 * (mcedm_cond_ddim_dxcond_workspace_bytes): as for mcedm_vp_heun_sample_dxcond.  mcedm_cond_ddim_sample[_rng|_guided] keep refusing
 * dx_cond plans. */
int mcedm_cond_ddim_dxcond_workspace_bytes(const mcedm_plan* plan, int B, int H, int W, size_t* bytes);
int mcedm_cond_ddim_sample_dxcond(const mcedm_plan* plan, const void* packed, const mcedm_cond_ddim_desc* sp,
                                  const mcedm_guidance_desc* dxc, const mcedm_guidance_desc* gd, const float* cond,
                                  const float* init_noise, const float* eta_noise, const uint64_t* rng_seed, float* xs_out,
                                  float* x0_out, int return_last, void* workspace, size_t workspace_bytes, int B, int H, int W,
                                  void* stream);

/* ---- kernel-level entry points ----------------------------------------------------------
 * The building blocks the schedules above are made of, exported so that each kernel can be
 * parity-tested against the oracle and timed on its own (bench.py roofline leg). */

/* Per-(sample, channel) input transform a conv applies while staging: v' = act((v-mean)*scale+offset). */
typedef struct { float mean, scale, offset, pad; } mcedm_coef;

/* Packed-weight size (floats) of a [Cout, Cin, k, k] conv, k in {1, 3}; bias_pk needs ceil32(Cout) floats. */
size_t mcedm_op_conv_packed_floats(int Cout, int Cin, int k);
/* Conv2d weights -> MFMA slab order.  qkv_heads > 0 re-orders output rows from the reference's
 * (head, c, {q,k,v}) interleave (adm_blocks.py:175) to (head, {q,k,v}, c).  dgrad != 0 packs the
 * transposed, tap-mirrored weights of the data gradient instead (then wpk has Cin output rows). */
int mcedm_op_pack_conv(const float* w, const float* b, int Cout, int Cin, int k, int qkv_heads, int dgrad,
                       float* wpk, float* bias_pk, void* stream);
/* GroupNorm statistics of cat(xa, xb) [B, Ca+Cb, HW] -> coef table [B][C] (models/adm_blocks.py:86-97
 * fused with the FiLM of :163-166 when film != NULL: row n = film[n*film_stride + (scale[0..C) | shift[C..2C))]).
 * groups = min(32, C/4).  stats_out [B][groups][2] (mean, rstd) may be NULL. */
int mcedm_op_gn_coef(const float* xa, const float* xb, int Ca, int Cb, int B, int HW, const float* gamma,
                     const float* beta, const float* film, int film_batch, int film_stride, float eps,
                     mcedm_coef* coef_out, float* stats_out, void* stream);
/* out = conv_k(resample(act(coef(cat(xa, xb))))) + bias + resample(res)   (models/adm_blocks.py:57-82 with the
 * pointwise ops of :161,166,171,179 fused).  resample / res_mode: 0 none, 1 nearest-2x up, 2 2x2-mean down.
 * resample 3 (k = 3 only, no residual): the conv itself has stride 2 over the source padded by one zero row / column at
 * the bottom / right -- the DDPM Downsample of models/ddim_blocks.py:85-104; then (Hs, Ws) = (2H, 2W).
 * (Hs, Ws) is the source size, (H, W) the conv size. */
int mcedm_op_conv(const float* xa, const float* xb, int Ca, int Cb, const mcedm_coef* coef, int coef_batch, int act,
                  int resample, int Hs, int Ws, int H, int W, const float* wpk, const float* bias_pk,
                  const float* res, int res_mode, float* out, int Cout, int B, int k, void* stream);
/* The same convolution (3x3, pad 1) in Winograd F(2x2, 3x3) form: 4/9 of the matrix instructions of mcedm_op_conv.
 * Serves Cout % 64 == 0, H % 8 == 0, W % 16 == 0, Ca % 8 == 0, Cb % 8 == 0, resample 0 (none) or 1 (nearest-2x up: the
 * source is [.., H/2, W/2]), res_mode 0, 1 (residual [.., H/2, W/2]) or 2 (2x2 mean of a residual [.., 2H, 2W]); results agree with mcedm_op_conv to fp32 rounding (a different
 * summation), not bit for bit.  w [Cout][Cin][3][3] -> wino (mcedm_op_conv_wino_packed_floats floats); bias [Cout] in
 * natural order or NULL; (H, W) is the conv (= output) size. */
size_t mcedm_op_conv_wino_packed_floats(int Cout, int Cin);
int mcedm_op_pack_conv_wino(const float* w, int Cout, int Cin, float* wino, void* stream);
int mcedm_op_conv_wino(const float* xa, const float* xb, int Ca, int Cb, const mcedm_coef* coef, int coef_batch, int act,
                       int resample, int H, int W, const float* wino, const float* bias, const float* res, int res_mode,
                       float* out, int Cout, int B, void* stream);
/* The same launch with the fused GroupNorm records of out in gsum: B * ceil(H / 4) * ceil(W / 8) * ceil(Cout / 4) * 2 floats (4-channel
 * blocks, as a plan's convs write them; kernel-level tests compare the records of two variants of the kernel). */
int mcedm_op_conv_wino_sums(const float* xa, const float* xb, int Ca, int Cb, const mcedm_coef* coef, int coef_batch, int act,
                            int resample, int H, int W, const float* wino, const float* bias, const float* res, int res_mode,
                            float* out, float* gsum, int Cout, int B, void* stream);
/* The same conv on the SPLIT variant of the Winograd kernel (one 32-channel output block per workgroup, the sixteen positions split
 * over its eight waves; see mcedm_op_set_conv_wino_split), whatever that switch says: un-resampled, images below 32 x 32 with
 * H % 8 == 0 and W % 16 == 0, Cout % 32 == 0, Ca % 8 == 0, (Ca + Cb) % 8 == 0, res_mode 0 or 2, 16-byte aligned inputs and table.
 * Outputs and records carry the bits of mcedm_op_conv_wino / mcedm_op_conv_wino_sums on a shape that both serve. */
int mcedm_op_conv_wino_split(const float* xa, const float* xb, int Ca, int Cb, const mcedm_coef* coef, int coef_batch, int act,
                             int H, int W, const float* wino, const float* bias, const float* res, int res_mode, float* out, int Cout,
                             int B, void* stream);
int mcedm_op_conv_wino_split_sums(const float* xa, const float* xb, int Ca, int Cb, const mcedm_coef* coef, int coef_batch, int act,
                                  int H, int W, const float* wino, const float* bias, const float* res, int res_mode, float* out,
                                  float* gsum, int Cout, int B, void* stream);
/* mcedm_op_conv and mcedm_op_conv_wino_sums with a bias row PER SAMPLE: the bias is [B][bias_batch], bias_batch >= Cout floats
 * between the rows of consecutive samples (0: one row for the whole batch, the entries above).  Un-resampled 3x3 convolutions of
 * more than 4 output channels only, in the Winograd form with act = 1 (the form the DDPM U-Net's conv1 launches: its own
 * instantiation of the kernel); any other launch with bias_batch != 0 is MCEDM_ERR_INVALID, never a result without it.
 * Sample b of the result equals, bit for bit, the single-row entry on sample b with row b. */
int mcedm_op_conv_bias_batch(const float* xa, const float* xb, int Ca, int Cb, const mcedm_coef* coef, int coef_batch, int act,
                             int resample, int Hs, int Ws, int H, int W, const float* wpk, const float* bias_pk, int bias_batch,
                             const float* res, int res_mode, float* out, int Cout, int B, int k, void* stream);
int mcedm_op_conv_wino_sums_bias_batch(const float* xa, const float* xb, int Ca, int Cb, const mcedm_coef* coef, int coef_batch,
                                       int act, int resample, int H, int W, const float* wino, const float* bias, int bias_batch,
                                       const float* res, int res_mode, float* out, float* gsum, int Cout, int B, void* stream);
/* The Winograd table of the DATA GRADIENT of that convolution (the backward of models/adm_blocks.py:57-82: du = conv3x3 of dy
 * with the weights transposed over the channels and mirrored over the taps).  w is the FORWARD weight [Cout][Cin][3][3]; wino
 * holds mcedm_op_conv_wino_packed_floats(Cin, Cout) floats and is used as mcedm_op_conv_wino(dy, .., wino, NULL bias, ..,
 * Cout = Cin of the forward conv): Cin % 64 == 0 and Cout % 8 == 0 of the forward conv are then required there. */
int mcedm_op_pack_conv_wino_dgrad(const float* w, int Cout, int Cin, float* wino, void* stream);
/* sigma-embedding MLP + every block's FiLM rows in one launch (models/adm_blocks.py:192-199 PositionalEmbedding,
 * :367-379 mapping MLP with SiLU, :143,163-165 per-block affine):  emb = silu(W1 silu(W0 pe(labels) + b0) + b1),
 * film[n] = Waff emb[n] + baff.  labels [n]; w0, w1 [ch][ch] (out, in); waff [rows][ch] = the blocks' affine weights
 * concatenated; freqs_scratch [ch/2]; emb_out [n][ch] (may be NULL); film_out [n][rows]. */
int mcedm_op_embedding(const float* labels, int n, int ch, const float* w0, const float* b0, const float* w1,
                       const float* b1, const float* waff, const float* baff, int rows, float* freqs_scratch,
                       float* emb_out, float* film_out, void* stream);
/* a = softmax(q^T k / sqrt(64)) v per (sample, head) (models/adm_blocks.py:103-109,174-178);
 * qkv is [B][heads][3][64][T] (the packed qkv conv's output), out [B][heads*64][T]. */
int mcedm_op_attention(const float* qkv, float* out, int B, int heads, int T, void* stream);
/* The whole attention part of a 64-channel UNetBlock at 8 x 8 in one launch (models/adm_blocks.py:174-180):
 * z = proj(attention(qkv(group_norm(y)))) + y, y and z [B][64][8][8], 16 groups, one head.  wq_pk / bq_pk: mcedm_op_pack_conv of
 * qkv.weight / qkv.bias with qkv_heads = 1; wp_pk / bp_pk: the same of proj with qkv_heads = 0.  gsum: NULL, or B * 16 * 2 floats
 * that receive the fused GroupNorm records (sum, M2 about the group mean) of z per 4-channel group.  Always the fused kernel:
 * the plan's dispatch (MCEDM_ATTN_FUSED, mcedm_op_set_attn_fused) does not apply, as for mcedm_op_attention. */
int mcedm_op_attn_block64(const float* y, const float* gamma, const float* beta, float eps, const float* wq_pk,
                          const float* bq_pk, const float* wp_pk, const float* bp_pk, float* z, float* gsum, int B, void* stream);
/* Backward building blocks.
 * conv weight / bias gradient: dw [Cout, Cin, k, k], db [Cout] (may be NULL) for the conv described as in mcedm_op_conv
 * (the transformed input is rebuilt into the scratch first); scratch holds mcedm_op_wgrad_scratch_floats() floats; qkv_heads > 0:
 * dy rows are in packed qkv order.  Data gradient = mcedm_op_conv on weights packed with dgrad = 1. */
size_t mcedm_op_wgrad_scratch_floats(int Cout, int Cin, int k, int B, int H, int W);
int mcedm_op_conv_wgrad(const float* dy, const float* xa, const float* xb, int Ca, int Cb, const mcedm_coef* coef,
                        int coef_batch, int act, int resample, int Hs, int Ws, int H, int W, int Cout, int B, int k,
                        int qkv_heads, float* scratch, float* dw, float* db, void* stream);
/* Backward of resample(act(film(group_norm(cat(xa, xb))))): dact is the gradient w.r.t. the conv input (conv
 * resolution), coef / stats come from mcedm_op_gn_coef of the forward.  Writes (or accumulates into) dxa / dxb, adds
 * `add` (add_mode 1: source resolution [B, C, Hs, Ws]; 2: conv resolution, mapped back through the resampling),
 * and returns dgamma, dbeta [C] and, when film != NULL, dfilm rows (d scale | d shift) with stride dfilm_stride.
 * ab is a [B][C][2] scratch. */
int mcedm_op_gn_bwd(const float* dact, int resample, const float* xa, const float* xb, int Ca, int Cb, int Hs, int Ws,
                    int B, const mcedm_coef* coef, const float* stats, const float* gamma, const float* beta,
                    const float* film, int film_batch, int film_stride, int act, float* dxa, float* dxb, int accumulate,
                    const float* add, int add_mode, float* ab, float* dgamma, float* dbeta, float* dfilm,
                    int dfilm_stride, void* stream);
/* The same with `sync`: MCEDM_GN_SYNC_WORDS * B * groups 32-bit words (groups = min(32, C / 4)), ZERO on entry and left
 * zero on exit.  With them a (sample, group) slab of 64 KB or more is cut into pieces of 4096 elements whose workgroups keep them in
 * LDS between the two passes and exchange their partial sums through `sync` (round 5; without it such slabs take the two-pass
 * kernel).  What the plan's backward (mcedm_denoise_backward) passes from its workspace. */
#define MCEDM_GN_SYNC_WORDS 130
int mcedm_op_gn_bwd_sync(const float* dact, int resample, const float* xa, const float* xb, int Ca, int Cb, int Hs, int Ws,
                         int B, const mcedm_coef* coef, const float* stats, const float* gamma, const float* beta,
                         const float* film, int film_batch, int film_stride, int act, float* dxa, float* dxb, int accumulate,
                         const float* add, int add_mode, float* ab, float* dgamma, float* dbeta, float* dfilm,
                         int dfilm_stride, unsigned int* sync, void* stream);
/* Attention backward (models/adm_blocks.py:111-118): qkv / dqkv packed [B][heads][3][64][T]; a, da [B][heads*64][T];
 * lse_scratch holds B*heads*T*2 floats. */
int mcedm_op_attention_bwd(const float* qkv, const float* a, const float* da, float* dqkv, float* lse_scratch, int B,
                           int heads, int T, void* stream);
/* One step of mcedm_cond_ddim_sample's elementwise part on caller-owned tensors (all fp32):
 *   et = (w + 1) F - w Fu (Fu != NULL) or F;  x0 = (xt - et * s1) / s0;  xt_next = sa_next * x0 [+ c1 * noise] + c2 * et
 * xt, F, Fu, noise, xt_next [B, C, H, W]; x0 also goes to channels [cond_channels, cond_channels + C) of condp and condp_u
 * ([B, plan_cond_channels, H, W], either may be NULL) and to slot t_x0 of x0s [B, T_x0, H, W, C], xt_next to slot t_xs of xs
 * [B, T_xs, H, W, C] (either may be NULL). */
int mcedm_op_ddim_cond_step(const float* xt, const float* F, const float* Fu, const float* noise, double w, float s0, float s1,
                            float sa_next, float c1, float c2, float* xt_next, float* condp, float* condp_u, int cond_channels,
                            int plan_cond_channels, int B, int C, int H, int W, float* xs, int T_xs, int t_xs, float* x0s,
                            int T_x0, int t_x0, void* stream);
/* The same step with `noise` generated in the kernel: draw `draw` of mcedm_uniform_fill keyed by *rng_seed (device memory).  The
 * value of an element depends on (seed, draw, element index) only, not on whether the 16-byte or the scalar path computed it. */
int mcedm_op_ddim_cond_step_rng(const float* xt, const float* F, const float* Fu, const uint64_t* rng_seed, uint64_t draw, double w,
                                float s0, float s1, float sa_next, float c1, float c2, float* xt_next, float* condp, float* condp_u,
                                int cond_channels, int plan_cond_channels, int B, int C, int H, int W, float* xs, int T_xs,
                                int t_xs, float* x0s, int T_x0, int t_x0, void* stream);
/* Both forms in one signature (noise, or rng_seed and draw; at most one of the two pointers) plus the PDE-guidance term of
 * mcedm_cond_ddim_sample_guided: et = et - gw * dx before x0 (models/ddim.py:1502-1503), dx [B, 1, H, W], gw = fl(5 * s1) formed by
 * the caller.  dx given requires C == 1 (MCEDM_ERR_INVALID otherwise); dx NULL is the step above bit for bit and gw is not read. */
int mcedm_op_ddim_cond_step_guided(const float* xt, const float* F, const float* Fu, const float* noise, const uint64_t* rng_seed,
                                   uint64_t draw, const float* dx, float gw, double w, float s0, float s1, float sa_next, float c1,
                                   float c2, float* xt_next, float* condp, float* condp_u, int cond_channels, int plan_cond_channels,
                                   int B, int C, int H, int W, float* xs, int T_xs, int t_xs, float* x0s, int T_x0, int t_x0,
                                   void* stream);
/* The two kernels of the training step's dropout (mcedm_unet_plan_set_dropout states the mask contract) on caller-owned tensors:
 *   out = mask * s * silu((h - mean) * scale + offset)   h, out [B, C, H, W]; coef [coef_batch ? B : 1][C] rows (mean, scale,
 *                                                        offset, pad), NULL = identity rows
 *   g   = mask * s * g                                   in place, g [B, C, H, W]
 * with mask and s = 1 / (1 - p) of draw `draw` keyed by *rng_seed (device memory).  0 < p < 1. */
int mcedm_op_dropout_act(const float* h, const mcedm_coef* coef, int coef_batch, float* out, int B, int C, int H, int W, double p,
                         const uint64_t* rng_seed, uint64_t draw, void* stream);
int mcedm_op_dropout_scale(float* g, int B, int C, int H, int W, double p, const uint64_t* rng_seed, uint64_t draw, void* stream);
/* Test hook: force the conv tile (channel tile mt in {32,64,128}, pixel tile ph x pw in {8x32,8x16,16x16,8x8};
 * (128,16,32) = the 8-wave kernel, 3x3 only);
 * (0,0,0) restores the size heuristic.  Process-global, not thread-safe. */
int mcedm_op_set_conv_tile(int mt, int ph, int pw);
/* Selects the experimental 8-wave conv kernel (one 512-thread workgroup per CU, double-buffered LDS slabs) for the
 * 3x3 layers large enough to give every CU a workgroup: 1 on, 0 off, -1 back to the default (env MCEDM_CONV8, else
 * off).  Results are bit-identical to the default kernel.  Process-global, not thread-safe. */
int mcedm_op_set_conv8(int enable);
/* The input-resident conv kernels that serve <= 32 x 32 images (conv_resident.hip: the tile's K extent in LDS by DMA,
 * weights streamed under the MFMAs): 1 on, 0 off (every conv takes conv_mfma_kernel), -1 back to the default (env
 * MCEDM_CONV_RESIDENT, else on).  Bit-identical to conv_mfma_kernel per tile configuration except the K-split tile used
 * at <= 8 x 8 (same result for a given shape, grouped differently).  Process-global, not thread-safe. */
int mcedm_op_set_conv_resident(int enable);
/* The Winograd F(2x2, 3x3) kernels (conv_wino.hip) in the network paths: 1 on, 0 off (direct kernels everywhere), -1 back to
 * the default (env MCEDM_WINOGRAD, else on).  Read when a plan lays out its workspace (whether a block's 1x1 skip projection
 * is folded into conv1 depends on it) and at every launch: set it before mcedm_unet_plan_create / the first forward.
 * Process-global, not thread-safe. */
int mcedm_op_set_conv_wino(int enable);
/* Which of the two Winograd kernels serves the 128-channel shapes: 1 = the one-wave-per-SIMD kernel (conv_wino1.hip: all 16
 * positions of a 32-channel block in one wave's AccVGPRs), 0 = the two-waves-per-SIMD kernel (conv_wino.hip), -1 = the default
 * (env MCEDM_WINO1, else 0: the one-wave kernel measured 6-9 % slower and stays off).  The two are bit-identical (statistics
 * included).  Read at every launch.  Process-global. */
int mcedm_op_set_conv_wino1(int enable);
/* The Winograd F(3x3, 2x2) weight-gradient kernel (wgrad_wino.hip) for the un-resampled 3x3 convs whose channel counts are
 * multiples of 128 on images with W % 32 == 0: 1 on, 0 off (the direct split-K kernel everywhere), -1 back to the default (env
 * MCEDM_WGRAD_WINO, else on).  Read at every launch; the scratch size does not depend on it.  Process-global. */
int mcedm_op_set_wgrad_wino(int enable);
/* The register-direct GEMM kernel (conv1x1_reg.hip) for 1x1 convs without input transform (the decoder blocks' skip projections and
 * their data gradients; Cout % 128 == 0, Cin % 16 == 0, Cin <= 256, H * W % 512 == 0): 1 on, 0 off (conv_mfma_kernel), -1 back to the
 * default (env MCEDM_CONV1X1_REG, else on).  Results differ from conv_mfma_kernel's in the last bits only through ... nothing: both sum
 * over ci in ascending pairs; tests hold them to rtol 1e-5.  Read at every launch.  Process-global. */
int mcedm_op_set_conv1x1_reg(int enable);
/* The SKIP variant of the Winograd kernel (conv_wino.hip): conv1 of an un-resampled decoder block computes the block's 1x1 skip
 * projection (Cout % 128 == 0, both sources % 16 == 0, 32 <= Cin <= 256) in its epilogue instead of reading it back from a launch
 * of its own: 1 on, 0 off, -1 back to the default (env MCEDM_WINO_FOLD, else on).  Bit-identical results either way (the
 * projection is summed in conv1x1_reg_kernel's order).  Read at every launch and at every forward; the workspace layout does not depend on it (the
 * projected tensor stays reserved), so it may change between calls on one workspace.  Process-global. */
int mcedm_op_set_conv_wino_fold(int enable);
/* The zero-position variant of the up-sampling Winograd kernel (conv_wino.hip, WinoUp): the input of an RS_UP conv is the nearest
 * 2x up-sampling of its source and every tile starts on an even pixel, so rows (and columns) 1 and 2 of every 4 x 4 input patch are
 * equal and the transformed input is exactly +0 at the seven Winograd positions with xi = 2 or nu = 2; the variant loads no weights,
 * reads no B fragments and issues no matrix instructions for them, and stages and transforms the tile's input at source resolution
 * (one load and one activation per source pixel): 1 on, 0 off (all sixteen positions), 2 the positions alone on the
 * sixteen-position kernel's staging (A/B runs; this hook and the environment only), -1 back to the default (env MCEDM_WINO_UPZ, else
 * on).  Bit-identical results in every form for finite transformed weights (a product with an exact zero is dropped instead of
 * yielding NaN).  Read at every launch; the workspace layout does not depend on it.  Process-global. */
int mcedm_op_set_conv_wino_upz(int enable);
/* The SPLIT variant of the Winograd kernel (conv_wino.hip, WinoSplitCfg) for the un-resampled 3x3 convs of images below 32 x 32 (the
 * 16 x 16 level) that carry a Winograd table: a workgroup is one 32-channel output block x one 8 x 16-pixel tile x all sixteen
 * positions, the positions split over its eight waves: 1 on, 0 off (the input-resident / tiled kernels, as before), -1 back to the
 * default (env MCEDM_WINO_SPLIT, else on).  Launches with a folded skip projection, a bias row per sample, the 8 x 8 level and
 * misaligned inputs keep their kernels, as does every launch while the input-resident switch or a tile is set explicitly, the
 * training path and the DDPM U-Net.  Results differ from the direct form in the last bits, as the Winograd kernel's do.  Read at every launch; the
 * workspace layout does not depend on it.  Process-global. */
int mcedm_op_set_conv_wino_split(int enable);
/* [Cout][Cin] weights of a 1x1 conv -> the MFMA-fragment order that mcedm_op_conv_skip's sk_wfrag expects;
 * wfrag holds ((Cout + 31) / 32 * 32) * ((Cin + 7) / 8 * 8) floats, 16-byte aligned. */
int mcedm_op_pack_conv_frag(const float* w, int Cout, int Cin, float* wfrag, void* stream);
/* conv1 of a decoder block as a plan launches it (through the dispatcher): out[B, Cout, H, W] = conv3x3(act(coef(x))) + bias + either
 * the residual res (same shape) or, with sk_wpk set, the folded 1x1 projection sk_bias + W * cat(sk_xa, sk_xb) (sk_wpk / sk_bias from
 * mcedm_op_pack_conv with k = 1; sk_wfrag from mcedm_op_pack_conv_frag or NULL, without which the Winograd kernel does not take
 * the fold).  wino: mcedm_op_pack_conv_wino's table or NULL.  gsum: NULL, or B * ceil(H / 4) * ceil(W / 8) * ceil(Cout / 4) * 2
 * floats that receive the fused GroupNorm records of out. */
int mcedm_op_conv_skip(const float* x, int Cin, const mcedm_coef* coef, int act, int H, int W, const float* wpk, const float* wino,
                       const float* bias, const float* res, const float* sk_xa, const float* sk_xb, int sk_Ca, int sk_Cb,
                       const float* sk_wpk, const float* sk_wfrag, const float* sk_bias, float* out, float* gsum, int Cout, int B,
                       void* stream);
/* The fused GroupNorm chain at kernel level.  A conv that produces a normalised tensor writes, per sample, pixel tile and block of rc
 * channels, a record (sum, M2 about the record's own mean); the next conv merges the records in fp64.  A tiling is five ints, the
 * geometry of a table: {tiles per sample, tiles along W, tile height, tile width, rc}; a table is [B][tiles][C / rc][2] floats.
 *
 * mcedm_op_conv_sums: the conv of mcedm_op_conv_bias_batch through the same dispatcher (wino: mcedm_op_pack_conv_wino's table or NULL,
 * with which the Winograd kernels may serve the launch as in a plan), with the records of out in gsum -- room for
 * B * ceil(H / 4) * ceil(W / 8) * (Cout / rc) * 2 floats, rc = 2 for gsum_rc = 2 and 4 for gsum_rc = 0 or 4 -- and the tiling the
 * launcher chose in tiling_out.  MCEDM_ERR_INVALID for a NULL gsum or tiling_out, any other gsum_rc, Cout % rc != 0 (no partial
 * records), and a kernel that cannot write the record width asked for. */
int mcedm_op_conv_sums(const float* xa, const float* xb, int Ca, int Cb, const mcedm_coef* coef, int coef_batch, int act, int resample,
                       int Hs, int Ws, int H, int W, const float* wpk, const float* wino, const float* bias_pk, int bias_batch,
                       const float* res, int res_mode, float* out, int Cout, int B, int k, float* gsum, int gsum_rc, int* tiling_out,
                       void* stream);
/* gn_coef_from_sums_kernel: coef_out [B][Ca + Cb] (and stats_out [B][groups][2] = (mean, rstd), or NULL) of GroupNorm(groups) (+ FiLM as in
 * mcedm_op_gn_coef) over cat(a, b) [B, Ca + Cb, H, W] from the records suma / sumb with tilings tiling_a / tiling_b (sumb, tiling_b NULL
 * iff Cb == 0).  MCEDM_ERR_INVALID unless each tiling covers H x W and every group is a whole number of records of each table it
 * touches: this entry never falls back to a pass over the tensor. */
int mcedm_op_gn_coef_from_sums(const float* suma, const float* sumb, const int* tiling_a, const int* tiling_b, int Ca, int Cb, int B, int H,
                               int W, int groups, const float* gamma, const float* beta, const float* film, int film_batch,
                               int film_stride, float eps, mcedm_coef* coef_out, float* stats_out, void* stream);
/* mcedm_op_conv whose transform rows are derived inside the kernel from the records of its SOURCE cat(xa, xb) [B, Ca + Cb, Hs, Ws]
 * (the inference path of both U-Nets: no GroupNorm kernel runs); arguments as in the two entries above. */
int mcedm_op_conv_gn(const float* xa, const float* xb, int Ca, int Cb, const float* suma, const float* sumb, const int* tiling_a,
                     const int* tiling_b, int groups, const float* gamma, const float* beta, const float* film, int film_batch,
                     int film_stride, float eps, int act, int resample, int Hs, int Ws, int H, int W, const float* wpk, const float* wino,
                     const float* bias_pk, const float* res, int res_mode, float* out, int Cout, int B, int k, void* stream);
/* The single-launch attention part of a UNetBlock at 8 x 8 x 64 channels (attn_fused.hip; inference only): 1 on, 0 off
 * (qkv conv + attention kernel + proj conv), -1 back to the default (env MCEDM_ATTN_FUSED, else on).  Process-global. */
int mcedm_op_set_attn_fused(int enable);
/* Diagnostics: when buf != NULL every conv workgroup writes 16 x u64 at buf[16*blockIdx]: [0..3] timestamps (10 ns
 * units) at start / first chunk / end of K loop / end of epilogue, [4] (XCC id << 32 | HW_ID), [5..6] shader-clock
 * counter at the K loop's ends, [8..] per-phase cycle sums (MCEDM_CONV_TIMELINE builds) or per-wave HW_ID (8-wave
 * kernel).  NULL switches it off. */
int mcedm_op_set_conv_debug(unsigned long long* buf);

/* ---- RePaint-style EDM sampling on the DDPM U-Net ---------------------------------------
 * The joint-DDPM baseline PlDdim (models/ddim.py) sampled with the EDM Heun sampler and RePaint-style resampling:
 * `sample_edm` (ddim.py:959-1051: n_repeat inner loops per step, the known region re-noised to the current level
 * after every loop), `get_denoised` (:915-947, VP preconditioning c_skip 1, c_out -sigma, c_noise = the nearest DDPM
 * timestep), `round_sigma` (:949-957), `compute_alpha` (:700-704), on the ermongroup/ddim U-Net `Model`
 * (models/ddim_blocks.py:222-470; configs/model/ddim_res32.yaml).  Inference only, one noise level per call,
 * cond = None, x_self_cond = None (zeros), dx = None -- exactly what sample_edm evaluates. */
typedef struct {
  int32_t in_channels;       /* hparams.model.in_channels (state channels h_ch + u_ch), 2 */
  int32_t out_channels;      /* out_ch */
  int32_t ch;                /* base width (multiple of 32); temb width is 4 * ch */
  int32_t n_levels;
  int32_t ch_mult[MCEDM_MAX_LEVELS];
  int32_t num_res_blocks;
  int32_t resolution;        /* the network asserts input size == resolution (ddim_blocks.py:411); levels are resolution >> l */
  int32_t n_attn_resolutions;
  int32_t attn_resolutions[MCEDM_MAX_LEVELS];
  int32_t self_cond;         /* 1: conv_in takes cat(x_self_cond, x) (ddim_blocks.py:262, 366-370) */
  float eps;                 /* GroupNorm eps, 1e-6 (ddim_blocks.py:62-63) */
} mcedm_ddpm_desc;

/* configs/diff_sampler/edm_sampler_inv.yaml + the diffusion schedule tables PlDdim derives from `betas`
 * (host pointers, fp32 as the reference holds them): edm_steps[n] = get_edm_steps() (ddim.py:131-137, largest sigma
 * first), alphas_cumprod_ext[n + 1] = cumprod(1 - cat(0, betas)) (the table compute_alpha indexes with t + 1). */
typedef struct {
  int32_t timesteps;
  double sigma_min, sigma_max, rho;
  double S_churn, S_min, S_max, S_noise;
  double w;                  /* must be 0 on this path (cond is None) */
  int32_t n_repeat;          /* resampling loops per step */
  int32_t n_time_h, n_time_u;/* rows [0, n_time_*) of the h / u channels are KNOWN (conditioning) */
  int32_t h_ch, u_ch;
  int32_t num_diffusion_timesteps;
  const float* edm_steps;
  const float* alphas_cumprod_ext;
} mcedm_repaint_desc;

typedef struct mcedm_ddpm_plan mcedm_ddpm_plan;
int mcedm_ddpm_plan_create(const mcedm_ddpm_desc* desc, mcedm_ddpm_plan** out);
void mcedm_ddpm_plan_destroy(mcedm_ddpm_plan* plan);
int mcedm_ddpm_plan_set_variant(mcedm_ddpm_plan* plan, int which, int value);      /* as mcedm_unet_plan_set_variant */
/* Parameter table in Model.state_dict() order (names as the reference's: "temb.dense.0.weight", "down.0.block.0.norm1.weight", ...). */
int mcedm_ddpm_param_count(const mcedm_ddpm_plan* plan);
int mcedm_ddpm_param_info(const mcedm_ddpm_plan* plan, int index, const char** name, int64_t* numel, int32_t* ndim,
                          int64_t shape[4]);
int mcedm_ddpm_packed_bytes(const mcedm_ddpm_plan* plan, size_t* bytes);
/* temb_freqs: device array [ch / 2] = exp(arange(ch/2) * -(ln 10000 / (ch/2 - 1))) exactly as get_timestep_embedding
 * builds it (ddim_blocks.py:22-24); the caller owns that expression because t * freqs reaches ~1000 and a 1-ulp
 * difference in a frequency is a 1e-4 difference in sin / cos. */
int mcedm_ddpm_pack_weights(const mcedm_ddpm_plan* plan, const float* const* params, const float* temb_freqs, void* packed,
                            void* stream);
int mcedm_ddpm_workspace_bytes(const mcedm_ddpm_plan* plan, int B, size_t* bytes);
/* Model.forward(x, t) (ddim_blocks.py:410-470), one timestep t for the whole batch; x [B, in_channels, R, R]. */
int mcedm_ddpm_forward(const mcedm_ddpm_plan* plan, const void* packed, const float* x, float t, float* out, void* workspace,
                       size_t workspace_bytes, int B, void* stream);
/* PlDdim.get_denoised at a scalar sigma: D = x - sigma * F(x / sqrt(sigma^2 + 1), c_noise); c_noise is the timestep
 * num_timesteps - 1 - round_sigma(sigma, return_index) the caller (or mcedm_repaint_sample) derives.  F_out may be NULL. */
int mcedm_ddpm_denoise(const mcedm_ddpm_plan* plan, const void* packed, const float* x, float sigma, float c_noise,
                       float* D_out, float* F_out, void* workspace, size_t workspace_bytes, int B, void* stream);
/* Host helper: the rounded sigma schedule of ddim.py:982-986 (timesteps + 1 values, last = 0). */
int mcedm_repaint_schedule(const mcedm_repaint_desc* sp, double* t_steps);
/* PlDdim.sample_edm (ddim.py:959-1051), guide_dx False.
 *  hu           [B, C, R, R] fp32 normalised joint state ('b h w c' of cat(h, u) rearranged to NCHW, ddim.py:967-968)
 *  init_noise   [B, C, R, R] fp32            randn_like(hu) (:969), also the noise of every known-region re-noising
 *  step_noise   [timesteps][B, C, R, R] fp64  the per-step draw (:1004); may be NULL when no step raises sigma
 *  repeat_noise [timesteps][n_repeat - 1][B, C, R, R] fp64  the draw between inner loops (:1037); NULL iff n_repeat == 1
 *  out          fp64 [B, 1 or timesteps + 1, R, R, C] */
int mcedm_repaint_workspace_bytes(const mcedm_ddpm_plan* plan, int B, size_t* bytes);
int mcedm_repaint_sample(const mcedm_ddpm_plan* plan, const void* packed, const mcedm_repaint_desc* sp, const float* hu,
                         const float* init_noise, const double* step_noise, const double* repeat_noise, double* out,
                         int return_last, void* workspace, size_t workspace_bytes, int B, void* stream);
/* The same sampler with the per-step and per-loop noise GENERATED ON THE DEVICE instead of read from tensors (the
 * reference draws timesteps * n_repeat randn_like tensors per call, ddim.py:1004, 1037: 576 at BASELINE config 5):
 * Philox4x32-10 keyed by the 64-bit seed at *rng_seed (DEVICE memory, read by the kernels when they run, so one captured
 * HIP graph replays with fresh noise after the host rewrites the seed), counter = (element pair, draw index), Box-Muller
 * on 53-bit uniforms.  Draw index of step i: i * n_repeat (the :1004 draw), i * n_repeat + 1 + k (the :1037 draw after
 * inner loop k).  Statistically equivalent to, not the same stream as, torch.randn_like. */
int mcedm_repaint_sample_rng(const mcedm_ddpm_plan* plan, const void* packed, const mcedm_repaint_desc* sp, const float* hu,
                             const float* init_noise, const uint64_t* rng_seed, double* out, int return_last,
                             void* workspace, size_t workspace_bytes, int B, void* stream);
/* out[0 .. n) = the N(0, 1) values of draw `draw` of that generator (fp64). */
int mcedm_normal_fill(double* out, size_t n, const uint64_t* rng_seed, uint64_t draw, void* stream);
/* The UNIFORM stream of the same generator (the DDIM samplers' torch.rand_like draws): out[e], e in [0, n), is word e % 4 of the
 * Philox4x32-10 block with key = the seed at *rng_seed and counter (lo32(e / 4), hi32(e / 4), lo32(draw), hi32(draw) | 0x80000000),
 * as u = (word >> 8) * 2^-24 -- fp32, in [0, 1), exactly representable, torch.rand's 24-bit granularity.  The set top bit of the
 * counter keeps these blocks disjoint from every block of the normal stream (whose draw indices stay below 2^63) under the same
 * seed.  out needs no particular alignment. */
int mcedm_uniform_fill(float* out, size_t n, const uint64_t* rng_seed, uint64_t draw, void* stream);

/* Model.forward(x, t, x_self_cond) with the self-conditioning tensor given (ddim_blocks.py:417-420; NULL = zeros, i.e.
 * mcedm_ddpm_forward).  x_self_cond [B, in_channels, R, R]. */
int mcedm_ddpm_forward_sc(const mcedm_ddpm_plan* plan, const void* packed, const float* x, const float* x_self_cond, float t,
                          float* out, void* workspace, size_t workspace_bytes, int B, void* stream);
/* PlDdim.sample_with_repeat (models/ddim.py:808-913): the DDIM sampler with RePaint-style inner loops, guide_dx False,
 * dx_cond False.  Everything is fp32 like the reference.
 *  timesteps, skip_type (0 uniform, 1 quad: ddim.py:823-830), eta, n_repeat, n_time_h / n_time_u / h_ch / u_ch as in
 *  mcedm_repaint_desc; alphas_cumprod_ext: host table cumprod(1 - cat(0, betas)) with num_diffusion_timesteps + 1 entries.
 *  hu, init_noise  [B, C, R, R]      normalised joint state; randn_like(hu) (:832)
 *  eta_noise       [timesteps][B, C, R, R] or NULL: the torch.rand_like draws of :893 (UNIFORM in the reference), eta != 0 only
 *  self_cond       1: the previous x0 prediction is fed back as x_self_cond (hparams.model.self_cond), 0: never
 *  xs_out, x0_out  fp32 [B, 1 or timesteps + 1, R, R, C] / [B, 1 or timesteps, R, R, C] ('b t h w c', as the reference returns) */
typedef struct mcedm_ddim_desc {
  int32_t timesteps, skip_type;
  double eta;
  int32_t n_repeat, n_time_h, n_time_u, h_ch, u_ch, num_diffusion_timesteps, self_cond;
  const float* alphas_cumprod_ext;
} mcedm_ddim_desc;
int mcedm_ddim_workspace_bytes(const mcedm_ddpm_plan* plan, int B, size_t* bytes);
/* Host helper: the timestep sequence the sampler walks (models/ddim.py:823-830), exactly as the reference builds it --
 * range(0, n, n // timesteps) for uniform, [int(s) for s in np.linspace(0, sqrt(0.8 n), timesteps) ** 2] for quad, with
 * numpy.linspace's own arithmetic (arange * step, last sample pinned to the stop value).  *count = entries (uniform may
 * exceed `timesteps`); seq may be NULL to query the count, else capacity >= *count. */
int mcedm_ddim_timesteps(int num_diffusion_timesteps, int timesteps, int skip_type, int* seq, int capacity, int* count);
int mcedm_ddim_repaint_sample(const mcedm_ddpm_plan* plan, const void* packed, const mcedm_ddim_desc* sp, const float* hu,
                              const float* init_noise, const float* eta_noise, float* xs_out, float* x0_out, int return_last,
                              void* workspace, size_t workspace_bytes, int B, void* stream);
/* The same with rng_seed in place of eta_noise: step k (in the order the steps are walked) uses draw k of mcedm_uniform_fill,
 * generated inside the step kernel; feeding mcedm_ddim_repaint_sample the tensors mcedm_uniform_fill writes reproduces the call
 * bit for bit.  With |eta| <= 1e-10 the seed is never read.  A NULL rng_seed is MCEDM_ERR_INVALID; every other check is
 * mcedm_ddim_repaint_sample's. */
int mcedm_ddim_repaint_sample_rng(const mcedm_ddpm_plan* plan, const void* packed, const mcedm_ddim_desc* sp, const float* hu,
                                  const float* init_noise, const uint64_t* rng_seed, float* xs_out, float* x0_out,
                                  int return_last, void* workspace, size_t workspace_bytes, int B, void* stream);

/* ---- the conditioning head of Model (cond_enc / combine_enc, models/ddim_blocks.py:279-306, 401-421) -------------------
 * cat_cond False, cond_channels > 0 (configs/model/ddim_cond_h_res32.yaml):
 *   x_feat = combine_enc(cat(conv_in(cat(x_self_cond, x)), cond_enc(cond))),
 *   cond_enc = Conv1x1(cond_channels -> ch) -> GELU (erf) -> Conv3x3(ch -> ch, circular padding), combine_enc = Conv1x1(2 ch -> ch),
 *   cond None: ZERO features in place of cond_enc(cond).
 * combine_enc is linear, so with Wx, Wc the two halves of its weight the plan folds, at pack time (fp64, rounded once),
 *   x_feat = (Wx conv_in)(z) + M,   M = (Wc cond_enc.2) (*)circ GELU(cond_enc.0(cond)) + (Wx b_in + Wc b_enc2 + b_comb):
 * the map M [B, ch, R, R] depends on cond alone (mcedm_ddpm_cond_map: one launch, a sampler runs it once per call) and the
 * folded conv_in adds it before its GroupNorm statistics; without cond (zero features, so no b_enc2 either) conv_in adds the
 * vector Wx b_in + b_comb and no map is read.  A network
 * evaluation launches exactly what a plan without the head launches.  The parameter table gains cond_enc.0.*, cond_enc.2.*,
 * combine_enc.* behind conv_in.*, as Model.state_dict() orders them.
 * cat_cond != 0 with cond_channels > 0 (configs/model/edm_cond_h_res32.yaml; models/ddim_blocks.py:259, 386-391): no head; conv_in
 * reads cat(cond, x), its weight is [ch, cond_channels + in_channels, 3, 3] and the parameter table is that of a plan without
 * conditioning.  It needs desc->self_cond == 0; with self_cond it is not built: MCEDM_ERR_INVALID. */
typedef struct { int32_t cond_channels; int32_t cat_cond; } mcedm_ddpm_cond_desc;
int mcedm_ddpm_plan_create_cond(const mcedm_ddpm_desc* desc, const mcedm_ddpm_cond_desc* cond, mcedm_ddpm_plan** out);
/* map_out [B, ch, R, R] <- M(cond), cond [B, cond_channels, R, R]; the caller owns map_out. */
int mcedm_ddpm_cond_map(const mcedm_ddpm_plan* plan, const void* packed, const float* cond, float* map_out, int B, void* stream);
/* Model.forward(x, t, cond, x_self_cond) with the conditioning given as its map: x_self_cond NULL = zeros, cond_map NULL = cond
 * None.  On a plan without the head cond_map must be NULL and this is mcedm_ddpm_forward_sc. */
int mcedm_ddpm_forward_cond(const mcedm_ddpm_plan* plan, const void* packed, const float* x, const float* x_self_cond,
                            const float* cond_map, float t, float* out, void* workspace, size_t workspace_bytes, int B, void* stream);
/* mcedm_vp_heun_sample[_rng] on the DDPM U-Net with the head: same description, same contracts (fp64 state, the rounded schedule
 * from the host, guidance for |w| >= 1e-3 with cond given, _rng bit-equal to the tensor-fed form on mcedm_normal_fill's draws).
 * sp->cond_channels is the plan's cond_channels (cond given) or 0 (cond NULL); the map is computed once, inside the call;
 * x_self_cond is None in every evaluation (get_self_cond_edm, :1603-1605).  H = W = the plan's resolution. */
int mcedm_ddpm_vp_sampler_workspace_bytes(const mcedm_ddpm_plan* plan, int B, size_t* bytes);
int mcedm_ddpm_vp_heun_sample(const mcedm_ddpm_plan* plan, const void* packed, const mcedm_vp_sampler_desc* sp, const float* cond,
                              const float* init_noise, const double* step_noise, double* out, int return_last, void* workspace,
                              size_t workspace_bytes, int B, void* stream);
int mcedm_ddpm_vp_heun_sample_rng(const mcedm_ddpm_plan* plan, const void* packed, const mcedm_vp_sampler_desc* sp, const float* cond,
                                  const float* init_noise, const uint64_t* rng_seed, double* out, int return_last, void* workspace,
                                  size_t workspace_bytes, int B, void* stream);
/* mcedm_cond_ddim_sample[_rng] on the DDPM U-Net with the head: the x0 prediction of a step is the next step's x_self_cond
 * (sp->self_cond, which needs a plan built with self_cond); the guidance pass runs without the map, on the same x_self_cond. */
int mcedm_ddpm_cond_ddim_workspace_bytes(const mcedm_ddpm_plan* plan, int B, size_t* bytes);
int mcedm_ddpm_cond_ddim_sample(const mcedm_ddpm_plan* plan, const void* packed, const mcedm_cond_ddim_desc* sp, const float* cond,
                                const float* init_noise, const float* eta_noise, float* xs_out, float* x0_out, int return_last,
                                void* workspace, size_t workspace_bytes, int B, void* stream);
int mcedm_ddpm_cond_ddim_sample_rng(const mcedm_ddpm_plan* plan, const void* packed, const mcedm_cond_ddim_desc* sp, const float* cond,
                                    const float* init_noise, const uint64_t* rng_seed, float* xs_out, float* x0_out, int return_last,
                                    void* workspace, size_t workspace_bytes, int B, void* stream);
/* mcedm_vp_heun_sample_guided and mcedm_cond_ddim_sample_guided on the DDPM U-Net with the head (guide_dx=True of
 * PlCondDdim.sample_edm, models/ddim.py:1576-1578, 1589-1590, and of PlCondDdim.sample, :1499-1503; dx from get_dx_pde
 * :1424-1450): the same description, checks, gd == NULL case and noise forms; h is plane 0 of cond, the guided workspaces are the
 * unguided ones plus the gradient and the Darcy scratch.  H = W = the plan's resolution. */
int mcedm_ddpm_vp_guided_workspace_bytes(const mcedm_ddpm_plan* plan, int B, size_t* bytes);
int mcedm_ddpm_vp_heun_sample_guided(const mcedm_ddpm_plan* plan, const void* packed, const mcedm_vp_sampler_desc* sp,
                                     const mcedm_guidance_desc* gd, const float* cond, const float* init_noise,
                                     const double* step_noise, const uint64_t* rng_seed, double* out, int return_last,
                                     void* workspace, size_t workspace_bytes, int B, void* stream);
int mcedm_ddpm_cond_ddim_guided_workspace_bytes(const mcedm_ddpm_plan* plan, int B, size_t* bytes);
int mcedm_ddpm_cond_ddim_sample_guided(const mcedm_ddpm_plan* plan, const void* packed, const mcedm_cond_ddim_desc* sp,
                                       const mcedm_guidance_desc* gd, const float* cond, const float* init_noise,
                                       const float* eta_noise, const uint64_t* rng_seed, float* xs_out, float* x0_out,
                                       int return_last, void* workspace, size_t workspace_bytes, int B, void* stream);

/* ---- the single-task EDM model on a cat_cond plan (PlCondEdm on Model, models/ddim.py:1608-1773) ------------------------
 * mcedm_ddpm_forward_cat: Model.forward(x, t, cond) with cond [B, cond_channels, R, R] concatenated in front of the state by
 * conv_in's two source pointers (no copy, no extra launch); cond NULL = cond None, which reads as zeros (:387-390).  On a plan
 * without cat_cond channels cond must be NULL and this is mcedm_ddpm_forward.
 * mcedm_ddpm_edm_denoise: PlCondEdm.get_denoised (:1745-1763) at one noise level, fp32:
 *   c_skip = sd^2 / (sigma^2 + sd^2), c_out = sigma sd / sqrt(sigma^2 + sd^2), c_in = 1 / sqrt(sd^2 + sigma^2),
 *   F = net(c_in x, c_noise, cond) -- c_in scales the state only, cond enters unscaled -- and, for |w| >= 1e-3 with cond given,
 *   F = (1 + w) F - w net(c_in x, c_noise, None);  D = c_skip x + c_out F.
 * c_noise is the caller's fp32 ln(sigma) / 4.  F_out (optional) receives the blended F. */
int mcedm_ddpm_forward_cat(const mcedm_ddpm_plan* plan, const void* packed, const float* x, const float* cond, float t, float* out,
                           void* workspace, size_t workspace_bytes, int B, void* stream);
int mcedm_ddpm_edm_denoise(const mcedm_ddpm_plan* plan, const void* packed, const float* x, const float* cond, float sigma,
                           float c_noise, double w, double sigma_data, float* D_out, float* F_out, void* workspace,
                           size_t workspace_bytes, int B, void* stream);
/* PlCondDdim.sample_edm as PlCondEdm inherits it (:1532-1601) around mcedm_ddpm_edm_denoise: the description is
 * mcedm_vp_heun_sample's (t_steps, t_hat -- round_sigma is the identity here -- and c_noise = ln(sigma) / 4 at t_hat and at t_next,
 * all from the host; cond_channels = the plan's with cond, 0 with cond NULL), the contracts too (fp64 state, materialised or
 * device-generated churn draws, _rng bit-equal to the tensor-fed form on mcedm_normal_fill's draws, one capturable call).
 * gd (optional): PDE guidance, after every denoiser call dx = get_dx_log_prob(h, D) with h = cond[:, 0] and
 * d -= gd->weight * dx / t_hat in both stages (:1576-1578, 1589-1590); it needs in_channels == 1 and cond. */
int mcedm_ddpm_edm_sampler_workspace_bytes(const mcedm_ddpm_plan* plan, int B, size_t* bytes);
int mcedm_ddpm_edm_heun_sample(const mcedm_ddpm_plan* plan, const void* packed, const mcedm_vp_sampler_desc* sp, double sigma_data,
                               const mcedm_guidance_desc* gd, const float* cond, const float* init_noise, const double* step_noise,
                               double* out, int return_last, void* workspace, size_t workspace_bytes, int B, void* stream);
int mcedm_ddpm_edm_heun_sample_rng(const mcedm_ddpm_plan* plan, const void* packed, const mcedm_vp_sampler_desc* sp,
                                   double sigma_data, const mcedm_guidance_desc* gd, const float* cond, const float* init_noise,
                                   const uint64_t* rng_seed, double* out, int return_last, void* workspace, size_t workspace_bytes,
                                   int B, void* stream);

/* ---- one timestep (noise level) per sample on the DDPM U-Net: the noising pass of training, forward only -------------------
 * Training draws a t (PlDdim, PlCondDdim: models/ddim.py:276-278) or a sigma (PlCondEdm: :1717-1719) per sample.  The entries
 * above evaluate the network at one timestep per call: the term temb_proj(swish(temb)) is folded into conv1's bias vector of every
 * ResnetBlock.  These entries keep one such row set PER SAMPLE: a table [B][rows] in the workspace, of which the convolutions read
 * row set b for sample b.  t and sigma are read from DEVICE memory, never by the host: a call can be captured in a graph and
 * replayed after rewriting them in place.  Per sample the arithmetic and its order are those of the one-timestep entries: with
 * every t[b] equal, mcedm_ddpm_forward_t returns the bits of mcedm_ddpm_forward / _sc / _cond / _cat at that t, and a sample's
 * result does not depend on the rest of the batch.  There is no backward: these are for evaluation under no_grad.
 * mcedm_ddpm_temb_row_count: rows = the sum of the output channels of the network's ResnetBlocks.
 * mcedm_ddpm_temb_rows: rows_out [B][rows] (device), row r of sample b = temb_proj_r . swish(MLP(emb(t[b]))) + temb_proj.bias[r] +
 *   conv1.bias[r]; the rows are ordered as the *.temb_proj.weight entries of the parameter table (mcedm_ddpm_param_info), each
 *   block's output channels in order.
 * mcedm_ddpm_forward_t: Model.forward(x, t [B], cond, x_self_cond) on any of the three kinds of plan.  x_self_cond NULL = zeros;
 *   cond_map (of mcedm_ddpm_cond_map) belongs to a plan with the head, cond_cat [B, cond_channels, R, R] to a cat_cond plan, NULL =
 *   cond None; a pointer the plan has no use for is MCEDM_ERR_INVALID before any launch.
 * mcedm_ddpm_edm_denoise_t: PlCondEdm.model_precond (:1654-1666) with sigma [B] on the device; c_skip, c_out, c_in and
 *   c_noise = ln(sigma) / 4 are computed there in fp32 with the reference's expressions, c_in scales the state channels only,
 *   D = c_skip x + c_out F per sample; F_out (optional) receives F.  No guidance (training never uses it): for |w| >= 1e-3 use
 *   mcedm_ddpm_edm_denoise at one noise level.
 * mcedm_ddpm_workspace_bytes_t: what these two entries need (the table included); every other size query is unchanged. */
int mcedm_ddpm_temb_row_count(const mcedm_ddpm_plan* plan, int* rows);
int mcedm_ddpm_temb_rows(const mcedm_ddpm_plan* plan, const void* packed, const float* t, int B, float* rows_out, void* stream);
int mcedm_ddpm_workspace_bytes_t(const mcedm_ddpm_plan* plan, int B, size_t* bytes);
int mcedm_ddpm_forward_t(const mcedm_ddpm_plan* plan, const void* packed, const float* x, const float* x_self_cond,
                         const float* cond_map, const float* cond_cat, const float* t, float* out, void* workspace,
                         size_t workspace_bytes, int B, void* stream);
int mcedm_ddpm_edm_denoise_t(const mcedm_ddpm_plan* plan, const void* packed, const float* x, const float* cond, const float* sigma,
                             double sigma_data, float* D_out, float* F_out, void* workspace, size_t workspace_bytes, int B,
                             void* stream);

/* ---- PDE residuals (forward) ----------------------------------------------
 * Replace the tensor-op bodies of models/pde_loss.py; results are bit-identical to the PyTorch CPU path.
 * All tensors are fp32, channel-last (b, t, x, 2) = (h, u) for SWE and (b, s, s, 2) = (a, u) for Darcy.
 *   half_dt = (float)(0.5 * Tn / n_times), dx = x[1] - x[0] of SweFvLoss.gen_x (models/pde_loss.py:102-118, fp32).
 * mcedm_swe_fv_step      SweFvLoss.f_t_swp1d      models/pde_loss.py:131-165   out (b, t, x, 2)
 * mcedm_swe_fv_residual  SweFvLoss.calculate_loss models/pde_loss.py:211-225 (+ clamp of forward, :245-247)
 *                        scale2_* = normalizer.divide ** 2 (get_scaling, :197-209); out (b, t, x, 2)
 * mcedm_darcy_residual   DarcyLoss.calculate_loss models/pde_loss.py:30-54 and the division / clamp of forward
 *                        (:80-86): two_dx = (float)(2 * D / s), denom = (s-4)^2; out (b, s-4, s-4) */
int mcedm_swe_fv_step(const float* s, float* out, int B, int T, int X, float half_dt, float dx, void* stream);
/* mcedm_swe_fv_unroll    SweFvLoss.unroll_from_init models/pde_loss.py:167-182 and, with gt / loss given, the residual of
 *                        unroll_loss (:184-197): n_steps dependent steps of mcedm_swe_fv_step from one initial row per sample in
 *                        ONE launch (one workgroup per sample, the row held in LDS), bit-identical to the n_steps launches.
 *   ic    B rows of X (h, u) pairs, ic_sample_stride floats apart (>= 2 * X), so that pred[:, 0] of a (b, t, x, 2) tensor is read in
 *         place; it must not overlap out.
 *   out, gt, loss  (B, n_steps + 1, X, 2), contiguous; row 0 of out is ic, copied verbatim.
 *   gt and loss are both NULL (scale2_* ignored) or both given: loss = (out - gt)^2 / scale2 on every row, row 0 included,
 *         with neither the NaN -> 0 nor the clamp of mcedm_swe_fv_residual (the reference's unroll_loss has neither).
 *   half_dt = (float)(0.5 * Tn / n_steps) (NOT Tn / (n_steps + 1): unroll_from_init divides by the step count, :176), dx as above.
 * MCEDM_ERR_INVALID, before any launch, with a message that names the argument: ic or out NULL, only one of gt / loss, X outside
 * [1, MCEDM_SWE_UNROLL_MAX_X], n_steps < 0, B < 0, ic_sample_stride < 2 * X.  B == 0 is MCEDM_OK without a launch; n_steps == 0
 * copies ic (and fills loss).  Allocates nothing and does not synchronise. */
#define MCEDM_SWE_UNROLL_MAX_X 4096   /* two rows of (h, u) pairs in 64 KB of LDS */
int mcedm_swe_fv_unroll(const float* ic, size_t ic_sample_stride, float* out, const float* gt, float* loss,
                        int B, int n_steps, int X, float half_dt, float dx, float scale2_h, float scale2_u, void* stream);
/* The return_d=True branches (the guidance gradients; analytic adjoints of the stencils, models/pde_loss.py:231-242 and
 * :60-75): mcedm_swe_fv_guidance = d mean(calculate_loss(pred, gt)) / d pred, out (b, t, x, 2);
 * mcedm_darcy_guidance = d mean(L) / d pred or, calc_prob != 0, d mean(log(2 (1 - sigmoid(1e5 L)) + 1e-12)) / d pred,
 * out (b, s, s, 2), scratch holds b * (s-4)^2 floats.  NaNs of the gradient are returned as 0 like the reference's. */
int mcedm_swe_fv_guidance(const float* pred, const float* gt, float* out, int B, int T, int X, float half_dt, float dx,
                          float scale2_h, float scale2_u, void* stream);
int mcedm_darcy_guidance(const float* pred, float* out, float* scratch, int B, int S, float two_dx, int calc_prob,
                         void* stream);
int mcedm_swe_fv_residual(const float* pred, const float* gt, float* out, int B, int T, int X, float half_dt, float dx,
                          float scale2_h, float scale2_u, int clamp, void* stream);
int mcedm_darcy_residual(const float* pred, float* out, int B, int S, float two_dx, float denom, int clamp, void* stream);
/* The PDE term of training (PlCondEdm.training_step with pde_loss_lambda > 0, models/ddim.py:1726-1731 -> get_pde_loss
 * :1388-1422 with clamp_loss=True): value and gradient of
 *   pde_loss = sum_{b,t,x} w_b * sum_fields clamp(residual(x_unnorm, gt), max=1),   x_unnorm = (h * div_h + sub_h, D * div_u + sub_u)
 * with the residual of mcedm_swe_fv_residual (gd->system 1; H = time rows, W = cells) or mcedm_darcy_residual (system 2; one field).
 *   gd        system, half_dt, dx / two_dx, sub_*, div_* as for the guided sampler (scale2_* = div_*^2); weight = pde_loss_lambda
 *   D         [B, 1, H, W], the denoised output of the network
 *   h         the NORMALISED conditioning field: element (b, t, x) at h[b * h_sb + t * h_st + x * h_sx]
 *   gt        NULL: the state itself (x_gt_unnorm = x_unnorm, :1402-1403), so the gradient also flows through the target; or
 *             un-normalised channel-last (B, H, W, 2) data without a gradient (use_gt_pde).  Darcy ignores it like the reference.
 *   w         [B] in device memory or NULL (= 1): the factor on sample b's residual, in the value and the gradient alike.  With
 *             pde_loss_prop_t the reference's division (:1415-1416) broadcasts to (b, b, t, x): w_b = sum_i 1 / (sigma_i + 1) for every b.
 *   loss_out  1 fp32 (device): pde_loss, NOT multiplied by weight; summed in a fixed order through `scratch`
 *             (MCEDM_REDUCE_SCRATCH_BYTES, as for mcedm_edm_loss): no floating-point atomics, bitwise reproducible
 *   dD        [B, 1, H, W] or NULL (value only): dD += weight * d pde_loss / d D in place (on the buffer mcedm_edm_loss wrote),
 *             the div_u of the un-normalisation included.  Every thread owns its cell.  The gradient's NaNs are not zeroed (the
 *             reference zeroes them only in the return_d branch); the clamp passes the gradient at L <= 1 and blocks it at L > 1 / NaN.
 *   pde_scratch  Darcy with dD: mcedm_pde_train_scratch_bytes(gd, B, H, W) = B * (H-4)^2 floats; otherwise unused (may be NULL)
 * MCEDM_ERR_INVALID before any launch, with a message that names the argument: gd / D / h / loss_out NULL, an unknown gd->system,
 * an empty shape, a short or misaligned scratch, Darcy with H != W or H <= 4 or a short pde_scratch.  Allocates nothing and does
 * not synchronise. */
size_t mcedm_pde_train_scratch_bytes(const mcedm_guidance_desc* gd, int B, int H, int W);
int mcedm_pde_train_loss(const mcedm_guidance_desc* gd, const float* D, const float* h, int64_t h_sb, int64_t h_st, int64_t h_sx,
                         const float* gt, const float* w, int B, int H, int W, float* loss_out, float* dD, void* pde_scratch,
                         size_t pde_scratch_bytes, void* scratch, size_t scratch_bytes, void* stream);

/* ---- measurement ---------------------------------------------------------------------------
 * Per-launch timing with HIP event pairs recorded on the launch stream (bench.py's roofline leg).
 * mcedm_prof_report waits for the events, then writes a JSON array
 *   [{"name", "launches", "total_ms", "flops", "bytes"}, ...]   (flops / bytes: algorithmic sums)
 * into buf and clears the records.  Not for use under graph capture. */
int mcedm_prof_enable(int on);
int mcedm_prof_report(char* buf, size_t buflen);

#ifdef __cplusplus
}
#endif
#endif /* MCEDM_HIP_H_ */
