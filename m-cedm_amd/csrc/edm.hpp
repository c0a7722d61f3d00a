// edm.hpp -- launchers of the EDM preconditioning / Heun sampler kernels (edm.hip).
#pragma once
#include <cmath>
#include <vector>

#include "common.hpp"

namespace mcedm {

int launch_precond_prepare(const float* sigma_dev, float sigma_host, int use_host, int n, float sigma_data,
                           int cond_ch, int in_ch, int dx_ch, float* coefs4, float* c_noise, Coef* conv_in_coef,
                           hipStream_t stream);
int launch_precond_finish(const float* x, const float* F, const float* Fu, double w, const float* coefs4, int n_sigma,
                          size_t per_sample, size_t total, float* D, float* F_out, hipStream_t stream);
int launch_heun_init(const float* cond, int cond_ch, int in_ch, size_t hw, const float* mask, const float* noise,
                     double t0, size_t total, double* x, float* x32, hipStream_t s);
int launch_heun_churn(double* x, const double* eps, const float* mask, double c, size_t total, float* x32,
                      hipStream_t s);
// x += c * N(0, 1) with the noise generated in the kernel (Philox4x32-10 keyed by the 64-bit seed at *seed_dev, counter =
// (element pair, draw)); launch_normal_fill writes the same draw out as a tensor
int launch_heun_churn_rng(double* x, const unsigned long long* seed_dev, unsigned long long draw, double c, size_t total, float* x32,
                          hipStream_t s, const float* mask = nullptr);
int launch_normal_fill(double* out, const unsigned long long* seed_dev, unsigned long long draw, size_t total, hipStream_t s);
// out[e] = U[0, 1) in fp32, (word >> 8) * 2^-24 with word e % 4 of the Philox block at counter (e / 4, draw | 2^63): the draws of
// the DDIM step kernels (launch_ddim_next_rng, DdimCondStep::seed), disjoint from the normal generator's blocks
int launch_uniform_fill(float* out, const unsigned long long* seed_dev, unsigned long long draw, size_t total, hipStream_t s);
// Training-step dropout (mcedm_unet_plan_set_dropout): element e of [B, C, H, W] is kept iff u[e] >= (float)p, u = draw `draw` of
// launch_uniform_fill; kept values times 1.0f / (1.0f - (float)p), dropped values exactly 0.0f.
//   out = mask * s * silu((h - mean) * scale + offset), one coef row per (sample, channel) (coef_batch) or per channel; null = identity
int launch_dropout_act(const float* h, const Coef* coef, int coef_batch, float* out, int B, int C, int H, int W, double p,
                       const unsigned long long* seed_dev, unsigned long long draw, hipStream_t s);
//   g = mask * s * g in place
int launch_dropout_scale(float* g, size_t total, double p, const unsigned long long* seed_dev, unsigned long long draw, hipStream_t s);
// dxg / wgt / gdiv: optional PDE-guidance term of the single-task sampler, d -= (double)((wgt * dxg) / gdiv) formed in fp32
// (models/ddim.py:1577-1579, 1590-1591: `weight * dx / t_hat`, with t_hat in BOTH stages)
int launch_heun_euler(const double* x_hat, const float* D, const float* mask, double t_hat, double dt, size_t total,
                      double* d_cur, double* x_next, float* x32, hipStream_t s, const float* dxg = nullptr, float wgt = 0.f,
                      float gdiv = 1.f);
int launch_heun_correct(const double* x_hat, const double* d_cur, const float* D, const float* mask, double t_next,
                        double dt, size_t total, double* x_next, float* x32, hipStream_t s, const float* dxg = nullptr,
                        float wgt = 0.f, float gdiv = 1.f);
int launch_heun_store(const double* x, int C, size_t hw, int t, int T, size_t total, double* out, hipStream_t s);

// PDE guidance gradients (pde.hip): analytic adjoints of the residual stencils.  The two fields of the state may live in
// different tensors (the single-task models take h from the conditioning and u from the denoised state), so every field
// has its own base pointer and batch stride; row / column strides are shared.
struct GuideIO {
  const float* in[2]; const float* gt[2];     // state fields and the residual's target (SWE; usually the same tensors)
  long in_sb[2], st, sx;
  float* out[2]; long out_sb[2], out_st, out_sx;
  float sub[2], div[2];                       // un-normalisation x * div + sub applied while reading
  int mean;                                   // 1: write the mean of the two field gradients to out[0] only
  float scale = 1.f;                          // mean form only: out[0] = fl(scale * mean), one fp32 rounding on the finished mean
};
int launch_swe_guidance(const GuideIO& io, int B, int T, int X, float half_dt, float dx, float scale2_h, float scale2_u,
                        hipStream_t s);
int launch_darcy_guidance(const GuideIO& io, float* scratch, int B, int S, float two_dx, int calc_prob, hipStream_t s);

// ---- RePaint-style sampler on the DDPM U-Net (models/ddim.py:915-1051): VP preconditioning and known-region kernels
// D = x + (-sigma) * F                                                   (get_denoised, ddim.py:923-946: c_skip 1, c_out -sigma)
int launch_vp_finish(const float* x, const float* F, float sigma, size_t total, float* D, hipStream_t s);
// conv_in transform rows of the VP network input: n_self zero/self-conditioning channels pass, the state is scaled by c_in
int launch_vp_coef(float c_in, int n_self, int n_in, Coef* out, hipStream_t s);
// ---- VP sampler of the ADM U-Net (PlCondDdim.sample_edm, models/ddim.py:1532-1601)
// conv_in rows: all n_rows channels of cat(cond', x) scaled by c_in, n_plain rows behind them (the dx channels of a cat_dx
// plan, which arrive scaled) by 1; *label = c_noise
int launch_vp_prepare(float c_in, int n_rows, float c_noise, Coef* coef, float* label, hipStream_t s, int n_plain = 0);
// D = x + (-sigma) * F with F = (w + 1) F - w Fu when Fu != NULL                  (get_denoised, ddim.py:940-945)
int launch_vp_cfg_finish(const float* x, const float* F, const float* Fu, double w, float sigma, size_t total, float* D,
                         hipStream_t s);
// ---- EDM sampler of the DDPM U-Net (PlCondEdm on Model, models/ddim.py:1745-1763)
// D = c_skip * x + c_out * F with F = (w + 1) F - w Fu when Fu != NULL; F_out (optional, not F itself) <- the blended F
int launch_edm_cfg_finish(const float* x, const float* F, const float* Fu, double w, float c_skip, float c_out, size_t total,
                          float* D, float* F_out, hipStream_t s);
// one noise level per sample, sigma [B] in device memory: coef [B][n_front + n_in] <- identity on the n_front channels in front of
// the state, c_in(sigma_b) on the n_in state channels; c_noise [B] <- ln(sigma_b) / 4                     (models/ddim.py:1656-1661)
int launch_edm_prepare_t(const float* sigma, float sigma_data, int n_front, int n_in, int B, Coef* coef, float* c_noise, hipStream_t s);
// D = c_skip(sigma_b) x + c_out(sigma_b) F over `per` elements per sample; F_out (optional, not F itself) <- F        (:1665)
int launch_edm_finish_t(const float* x, const float* F, const float* sigma, float sigma_data, size_t per, size_t total, float* D,
                        float* F_out, hipStream_t s);
// x0 = ((hu*sa + nz*sb)*m + nz*(1-m)) [fp32] -> fp64, times t0       (ddim.py:989-994), m = 1 marks KNOWN entries
int launch_repaint_init(const float* hu, const float* noise, const float* mask, float sa, float sb, double t0, size_t total,
                        double* x, float* x32, hipStream_t s);
// x = (sa*hu + sb*nz)*m [fp32] + x*(1-m) [fp64]                          (ddim.py:1029-1031); final: x = hu*m + x*(1-m) (:1041-1043)
int launch_repaint_known(double* x, const float* hu, const float* noise, const float* mask, float sa, float sb, int final_clean,
                         size_t total, float* x32, hipStream_t s);

// ---- DDIM sampler with RePaint loops (PlDdim.sample_with_repeat, models/ddim.py:808-913), all fp32
// x0 = (xt - et * s1) / s0;  x0 = hu * m + x0 * (1 - m);  renoise: xt = s0 * x0 + s1 * et     (:873-882)
int launch_ddim_x0(float* xt, const float* et, const float* hu, const float* mask, float s0, float s1, int renoise, size_t total,
                   float* x0, hipStream_t s);
// xt_next = sa * x0 + [c1 * noise +] c2 * et;  xt_next = (sa * hu + c2 * hn) * m + xt_next * (1 - m)   (:884-895)
int launch_ddim_next(const float* x0, const float* et, const float* hu, const float* hn, const float* mask, const float* noise,
                     float sa, float c1, float c2, size_t total, float* xt, hipStream_t s);
// the stochastic step with `noise` = draw `draw` of launch_uniform_fill, generated in the kernel
int launch_ddim_next_rng(const float* x0, const float* et, const float* hu, const float* hn, const float* mask,
                         const unsigned long long* seed_dev, unsigned long long draw, float sa, float c1, float c2, size_t total,
                         float* xt, hipStream_t s);
// x = (hu * sa + hn * sb) * m + hn * (1 - m)   (:837-838)
int launch_ddim_init(const float* hu, const float* hn, const float* mask, float sa, float sb, size_t total, float* xt, hipStream_t s);
// 'b c h w -> b t h w c' for one time slot, fp32
int launch_store_f32(const float* x, int C, size_t hw, int t, int T, size_t total, float* out, hipStream_t s);

// The DDIM timestep sequence of PlDdim.sample_with_repeat / PlCondDdim.sample (models/ddim.py:823-830, 1463-1470).
//  uniform: range(0, n, n // N) -- may hold more than N entries;
//  quad:    [int(s) for s in np.linspace(0, sqrt(0.8 n), N) ** 2].  numpy.linspace evaluates arange(N) * step with
//           step = stop / (N - 1) and then PINS the last sample to `stop` itself; hi * i / (N - 1) is a different rounding
//           and lands on the other side of an integer for 85 of ~1200 (n, N) pairs (n = 1000, N = 100: first sampled step
//           799 instead of 800), so the two operations are reproduced in numpy's order.
static inline std::vector<int> ddim_timestep_seq(int n, int N, int skip_type) {
  std::vector<int> seq;
  if (skip_type == 0) {
    const int skip = n / N;
    for (int v = 0; v < n; v += skip) seq.push_back(v);
  } else {
    const double hi = std::sqrt(n * 0.8);
    const double step = N > 1 ? hi / (double)(N - 1) : 0.0;
    for (int i = 0; i < N; ++i) {
      const double v = (N > 1 && i == N - 1) ? hi : (double)i * step;
      seq.push_back((int)(v * v));
    }
  }
  return seq;
}

// ---- DDIM sampler of the conditional ADM U-Net (PlCondDdim.sample, models/ddim.py:1452-1530), all fp32: one step
//   et = w1 * F - w * Fu (Fu != NULL) or F;  x0 = (xt - et * s1) / s0;  xt_next = sa * x0 [+ c1 * noise] + c2 * et   (:1497-1515)
// in one pass that also puts x0 and xt_next where they are read next.  Every pointer but xt, F and xt_next may be NULL.
// seed != NULL (then noise is NULL): the kernel generates `noise` itself, draw `draw` of launch_uniform_fill keyed by *seed.
// dxg != NULL (C == 1): PDE guidance, et = et - gw * dxg before x0 (:1501-1503), gw = fl(5 * s1) formed by the caller.
struct DdimCondStep {
  const float *xt, *F, *Fu, *noise;        // [B, C, H, W]
  const unsigned long long* seed;          // device memory, read when the kernel runs
  unsigned long long draw;
  float w1, w, s0, s1, sa, c1, c2;
  const float* dxg;                        // [B, 1, H, W] get_dx_log_prob(h, xt), or NULL
  float gw;
  float* xt_next;                          // [B, C, H, W]
  float *sc, *sc_u;                        // [B, Cp, H, W] cond' and its zero-cond twin: x0 -> channels [sc_off, sc_off + C)
  int C, Cp, sc_off;
  size_t hw, n;                            // H * W;  B * C * H * W
  float *xs, *x0s;                         // 'b t h w c' trajectories: xt_next -> slot t_xs of T_xs, x0 -> slot t_x0 of T_x0
  int T_xs, t_xs, T_x0, t_x0;
};
int launch_ddim_cond_step(const DdimCondStep& a, hipStream_t s);

// ---- deterministic grid-wide sums (loss, gradient norm) ---------------------------------------------------------
// Every block stores its partial sum (fp64) in a slot of a scratch array, takes a ticket, and the block that draws the LAST
// ticket adds the slots in index order: the value does not depend on the order the blocks ran in (an atomicAdd of the
// partials would make the loss, the clip factor and with them the whole training run differ in the last bits from run to
// run).  The array and the ticket live in CALLER-owned scratch (ABI 3: MCEDM_REDUCE_SCRATCH_BYTES per concurrent call), so
// two plans on two streams of one device never share state; the entry point zeroes the ticket on the stream in front of
// the kernel.  Layout: [RED_MAX] fp64 partials, then the 32-bit ticket.
constexpr int RED_MAX = 4096;
static_assert(MCEDM_REDUCE_SCRATCH_BYTES >= RED_MAX * 8 + 4, "mcedm_hip.h: MCEDM_REDUCE_SCRATCH_BYTES too small for the reduction");
struct RedScratch { double* part; unsigned* ticket; };
static inline RedScratch red_scratch(void* scratch) {
  return RedScratch{reinterpret_cast<double*>(scratch), reinterpret_cast<unsigned*>(reinterpret_cast<char*>(scratch) + (size_t)RED_MAX * 8)};
}

// block_sum: this block's partial in thread 0.  Returns true in every thread of the LAST block, with the total in *total
// (thread 0 only).
__device__ __forceinline__ bool grid_sum_fixed_order(RedScratch rs, double block_sum, unsigned bid, unsigned nblocks, double* total) {
  __shared__ unsigned s_last;
  __shared__ double s_red[4];
  if (threadIdx.x == 0) {
    __hip_atomic_store(&rs.part[bid], block_sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __threadfence();
    s_last = (atomicAdd(rs.ticket, 1u) == nblocks - 1) ? 1u : 0u;
  }
  __syncthreads();
  if (!s_last) return false;
  __threadfence();
  double t = 0.0;
  for (unsigned i = threadIdx.x; i < nblocks; i += blockDim.x)      // fixed assignment of slots to threads
    t += __hip_atomic_load(&rs.part[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) t += __shfl_xor(t, off);
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = t;
  __syncthreads();
  if (threadIdx.x == 0) {
    *total = (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]);
    *rs.ticket = 0u;
  }
  return true;
}

}  // namespace mcedm
