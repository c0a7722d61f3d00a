// heun.hpp -- what the Heun samplers share (EDM and VP on the ADM U-Net: sampler.hip; RePaint, VP and EDM on the DDPM
// U-Net: ddpm.hip): the five state buffers in front of the network's workspace, the trajectory stores, the churn and the
// 2nd-order update.  Each sampler keeps its own schedule arithmetic (fp64, on the host), decides itself whether a step
// churns, and passes its network in as a callable.  The VP Heun loop and the conditional DDIM loop, which run on either
// network, are here whole (vp_heun_loop, cond_ddim_loop).
#pragma once
#include <cmath>
#include <utility>
#include <vector>

#include "edm.hpp"
#include "plan.hpp"

namespace mcedm {

// byte offsets of the fp64 state x, the next state xn, the Euler slope d, and of the fp32 network input x32 and output D
struct HeunBufs { size_t x, xn, d, x32, D, total; };
// a sampler's own buffers go behind the five: each take appends one, 256-byte aligned (any offset table with a `total`)
template <class Bufs>
static inline size_t heun_take(Bufs& b, size_t bytes) { size_t o = b.total; b.total += align_up(bytes, 256); return o; }
static inline HeunBufs heun_bufs(size_t n) {      // n = B * C * H * W state elements
  HeunBufs b{};
  b.x = heun_take(b, n * 8); b.xn = heun_take(b, n * 8); b.d = heun_take(b, n * 8);
  b.x32 = heun_take(b, n * 4); b.D = heun_take(b, n * 4);
  return b;
}

struct HeunState {
  double *x, *xn, *d;
  float *x32, *D;
  int C;
  size_t hw, total;
  int N, Tout, return_last;      // N steps; the trajectory has Tout = N + 1 slots, or 1 with return_last
  hipStream_t s;
  double* out;
};
static inline HeunState heun_state(void* ws, const HeunBufs& b, int B, int C, size_t hw, int N, int return_last, double* out,
                                   hipStream_t s) {
  return HeunState{at<double>(ws, b.x), at<double>(ws, b.xn), at<double>(ws, b.d), at<float>(ws, b.x32), at<float>(ws, b.D),
                   C, hw, (size_t)B * C * hw, N, return_last ? 1 : N + 1, return_last, s, out};
}

// trajectory slot `slot` <- x (0 after the init, i + 1 after step i); nothing with return_last, whose one store is the last
static inline int heun_store_step(const HeunState& h, int slot) {
  return h.return_last ? MCEDM_OK : launch_heun_store(h.x, h.C, h.hw, slot, h.Tout, h.total, h.out, h.s);
}
static inline int heun_store_last(const HeunState& h) {
  return h.return_last ? launch_heun_store(h.x, h.C, h.hw, 0, 1, h.total, h.out, h.s) : MCEDM_OK;
}

// x += c * eps (masked entries stay): eps = this step's materialised draws, or null for draw number `draw` of the device
// generator keyed by *seed
static inline int heun_churn(const HeunState& h, double c, const double* eps, const unsigned long long* seed,
                             unsigned long long draw, const float* mask) {
  if (eps) return launch_heun_churn(h.x, eps, mask, c, h.total, h.x32, h.s);
  return launch_heun_churn_rng(h.x, seed, draw, c, h.total, h.x32, h.s, mask);
}

// One Heun update of step i from x (= x_hat) at t_hat to t_next: Euler, then for every step but the last the 2nd-order
// correction; x is the new state afterwards.  denoise(sigma, is_second) leaves D(x32; sigma) in h.D (x32 holds x_hat for
// the first call, the Euler x_next for the second).  dxg / wgt / gdiv: the PDE-guidance term of launch_heun_euler.
template <class Denoise>
static inline int heun_update(HeunState& h, int i, double t_hat, double t_next, const float* mask, Denoise&& denoise,
                              const float* dxg = nullptr, float wgt = 0.f, float gdiv = 1.f) {
  int rc;
  if ((rc = denoise(t_hat, false))) return rc;
  if ((rc = launch_heun_euler(h.x, h.D, mask, t_hat, t_next - t_hat, h.total, h.d, h.xn, h.x32, h.s, dxg, wgt, gdiv)))
    return rc;
  if (i < h.N - 1) {
    if ((rc = denoise(t_next, true))) return rc;
    if ((rc = launch_heun_correct(h.x, h.d, h.D, mask, t_next, t_next - t_hat, h.total, h.xn, h.x32, h.s, dxg, wgt, gdiv)))
      return rc;
  }
  std::swap(h.x, h.xn);
  return MCEDM_OK;
}

// dx = get_dx_log_prob(h, denoised, guide_dx) of the single-task models (models/ddim.py:641-650 -> get_dx_pde :1424-1450):
// the residual of x_unnorm = (h from the conditioning, u = the denoised state), differentiated w.r.t. x_unnorm, then the
// MEAN over the two field gradients (calc_prob=True) -> [B, 1, H, W].  cond [B, cond_channels, H, W] of either network: its
// first plane is h.
// (the same call on the current noisy state instead of D is get_dx_input(h, x) with dx_norm == 'prob', ddim.py:601-613)
// scale: the stored value is fl(scale * dx), what PlCondDdim.get_denoised hands its network (c_in * dx, ddim.py:933-934)
static inline int guidance_dx(int cond_channels, const mcedm_guidance_desc& g, const float* cond, const float* D, float* dx,
                              float* scratch, int B, int H, int W, hipStream_t s, float scale = 1.f) {
  GuideIO io{};
  io.scale = scale;
  const long hw = (long)H * W;
  io.in[0] = cond; io.in[1] = D; io.gt[0] = cond; io.gt[1] = D;
  io.in_sb[0] = (long)cond_channels * hw; io.in_sb[1] = hw; io.st = W; io.sx = 1;
  io.out[0] = dx; io.out[1] = nullptr; io.out_sb[0] = hw; io.out_sb[1] = 0; io.out_st = W; io.out_sx = 1;
  io.sub[0] = g.sub_h; io.sub[1] = g.sub_u; io.div[0] = g.div_h; io.div[1] = g.div_u;
  io.mean = 1;
  if (g.system == 1)      // SweFvLoss: half_dt = 0.5 * Tn / n_times, dx = x[1] - x[0] of gen_x, both formed by the caller in fp32
    return launch_swe_guidance(io, B, H, W, g.half_dt, g.dx, g.div_h * g.div_h, g.div_u * g.div_u, s);
  MCEDM_REQUIRE(H == W && H > 4, "guidance: the Darcy residual needs a square grid larger than 4 x 4 (got %d x %d)", H, W);
  return launch_darcy_guidance(io, scratch, B, H, g.two_dx, /*calc_prob=*/1, s);
}

// ------------------------------------------------------------------------------------------
// PlCondDdim.sample_edm (models/ddim.py:1532-1601) on either network
// ------------------------------------------------------------------------------------------
// the checks of the schedule arrays; the caller has checked its plan and its pointers
static inline int vp_check_schedule(const mcedm_vp_sampler_desc* sp, const double* step_noise, const uint64_t* rng_seed) {
  MCEDM_REQUIRE(sp->timesteps >= 1 && sp->timesteps <= 4096, "vp_heun_sample: timesteps=%d out of range", sp->timesteps);
  for (int i = 0; i < sp->timesteps; ++i) {
    MCEDM_REQUIRE(sp->t_hat[i] >= sp->t_steps[i] && sp->t_steps[i] > 0.0, "vp_heun_sample: step %d: t_hat %g < t_cur %g or t_cur <= 0", i,
                  sp->t_hat[i], sp->t_steps[i]);
    MCEDM_REQUIRE(sp->t_hat[i] == sp->t_steps[i] || step_noise != nullptr || rng_seed != nullptr,
                  "vp_heun_sample: step %d churns (t_hat > t_cur) and needs step_noise (or mcedm_vp_heun_sample_rng)", i);
  }
  return MCEDM_OK;
}

// denoise(sigma, c_noise) leaves D(h.x32; sigma) in h.D: get_denoised (:915-947, PlCondEdm's :1745-1763) of the caller's
// network.  dxg / wgt: the PDE-guidance term, d -= wgt * dxg / t_hat in both stages (:1576-1578, 1589-1590); the callable
// leaves get_dx_log_prob(h, D) in dxg after every evaluation.
template <class Denoise>
static inline int vp_heun_loop(HeunState& h, const mcedm_vp_sampler_desc* sp, const float* init_noise, const double* step_noise,
                               const uint64_t* rng_seed, Denoise&& denoise, const float* dxg = nullptr, float wgt = 0.f) {
  int rc;
  const int N = sp->timesteps;
  const double* t = sp->t_steps;
  // x = u_noise.to(float64) * t_steps[0]   (:1556)
  if ((rc = launch_heun_init(nullptr, 0, h.C, h.hw, nullptr, init_noise, t[0], h.total, h.x, h.x32, h.s))) return rc;
  if ((rc = heun_store_step(h, 0))) return rc;
  for (int i = 0; i < N; ++i) {
    const double t_cur = t[i], t_next = t[i + 1], t_hat = sp->t_hat[i];
    if (t_hat != t_cur) {                 // x_hat = x_cur + sqrt(t_hat^2 - t_cur^2) * S_noise * eps (:1567); + 0 * eps otherwise
      const double c = std::sqrt(t_hat * t_hat - t_cur * t_cur) * sp->S_noise;
      if ((rc = heun_churn(h, c, step_noise ? step_noise + (size_t)i * h.total : nullptr,
                           reinterpret_cast<const unsigned long long*>(rng_seed), (unsigned long long)i, nullptr))) return rc;
    }
    // Euler step (:1570-1580) at c_noise[2 i], 2nd-order correction (:1583-1593) at c_noise[2 i + 1]
    auto at_level = [&](double sigma, bool second) { return denoise(sigma, sp->c_noise[2 * i + (second ? 1 : 0)]); };
    if ((rc = heun_update(h, i, t_hat, t_next, nullptr, at_level, dxg, wgt, dxg ? (float)t_hat : 1.f))) return rc;
    if ((rc = heun_store_step(h, i + 1))) return rc;
  }
  return heun_store_last(h);
}

// ------------------------------------------------------------------------------------------
// PlCondDdim.sample (models/ddim.py:1452-1530) on either network: fp32 throughout
// ------------------------------------------------------------------------------------------
static inline int cond_ddim_check_schedule(const mcedm_cond_ddim_desc* sp, const float* eta_noise, const uint64_t* rng_seed) {
  const int n = sp->num_diffusion_timesteps, N = sp->timesteps;
  MCEDM_REQUIRE(sp->alphas_cumprod_ext && n >= 2 && N >= 1 && N <= n, "cond_ddim_sample: bad schedule (timesteps=%d of %d)", N, n);
  MCEDM_REQUIRE(sp->skip_type == 0 || sp->skip_type == 1, "cond_ddim_sample: skip_type must be 0 (uniform) or 1 (quad)");
  MCEDM_REQUIRE(!(std::fabs(sp->eta) > 1e-10) || eta_noise != nullptr || rng_seed != nullptr, "cond_ddim_sample: eta != 0 needs eta_noise");   // :1509
  for (int t : ddim_timestep_seq(n, N, sp->skip_type))       // :1463-1470
    MCEDM_REQUIRE(t >= 0 && t < n, "cond_ddim_sample: timestep %d outside the schedule table", t);
  return MCEDM_OK;
}
static inline bool cond_ddim_guided(const mcedm_cond_ddim_desc* sp) { return !(std::fabs(sp->w) < 0.001); }      // :1493

// The noise coefficients of one DDIM step (:1509-1513, and :884-894 of sample_with_repeat), fp32 like the tensors:
// c1 = eta * sqrt((1 - at / at_next) * (1 - at_next) / (1 - at)); c2 = sqrt((1 - at_next) - c1^2); c1 = 0 when eta is
struct DdimNoiseCoefs { float c1, c2; };
static inline DdimNoiseCoefs ddim_noise_coefs(bool stochastic, double eta, float a_t, float at_next) {
  DdimNoiseCoefs k{0.f, 0.f};
  if (stochastic) {
    k.c1 = (float)eta * sqrtf((1.0f - a_t / at_next) * (1.0f - at_next) / (1.0f - a_t));
    k.c2 = sqrtf((1.0f - at_next) - k.c1 * k.c1);
  } else {
    k.c2 = sqrtf(1.0f - at_next);
  }
  return k;
}

// The state and network-output buffers of the loop, and where the step kernel leaves the x0 prediction for the next
// evaluation: channels [sc_off, sc_off + C) of sc (and of sc_u) [B, Cp, H, W]; sc null = no self-conditioning feedback.
struct CondDdimLoop {
  int C; size_t hw, total;
  float *xt, *xtn, *F, *Fu;            // Fu null = no guidance pass
  float *sc, *sc_u; int Cp, sc_off;
};
// net(xt, t, step) runs the network on xt under the label t into b.F (and, guided, without cond into b.Fu).
// dxg / wgt / pde: the PDE-guidance term, et -= fl(wgt * sqrt(1 - a_t)) * dxg (:1501-1503); pde(xt) leaves
// get_dx_log_prob(h, xt) of the CURRENT NOISY state in dxg.  xt of a step is known before its network runs, so the
// guidance launches go in front of the network's and the step kernel reads dxg.
template <class Net, class Pde>
static inline int cond_ddim_loop(const mcedm_cond_ddim_desc* sp, const CondDdimLoop& b, const float* init_noise, const float* eta_noise,
                                 const uint64_t* rng_seed, float* xs_out, float* x0_out, int return_last, hipStream_t s, Net&& net,
                                 const float* dxg, float wgt, Pde&& pde) {
  int rc;
  const std::vector<int> seq = ddim_timestep_seq(sp->num_diffusion_timesteps, sp->timesteps, sp->skip_type);   // walked from its end, seq_next = [-1] + seq[:-1]
  const int S = (int)seq.size();
  const bool stochastic = std::fabs(sp->eta) > 1e-10;                   // :1509
  if (!return_last && (rc = launch_store_f32(init_noise, b.C, b.hw, 0, S + 1, b.total, xs_out, s))) return rc;      // xs = [x]  (:1477)
  DdimCondStep k{};
  k.F = b.F; k.Fu = b.Fu;
  k.w1 = (float)(sp->w + 1.0); k.w = (float)sp->w;
  k.sc = b.sc; k.sc_u = b.sc_u;
  k.C = b.C; k.Cp = b.Cp; k.sc_off = b.sc_off; k.hw = b.hw; k.n = b.total;
  k.T_xs = return_last ? 1 : S + 1; k.T_x0 = return_last ? 1 : S;
  k.dxg = dxg;
  const float* xt = init_noise;
  float* bufs[2] = {b.xtn, b.xt};
  auto alpha = [&](int t) -> float { return sp->alphas_cumprod_ext[t + 1]; };      // compute_alpha(t): index t + 1 (:700-704)
  for (int step = 0; step < S; ++step) {
    const int i = seq[S - 1 - step], j = (S - 1 - step) > 0 ? seq[S - 2 - step] : -1;
    const float a_t = alpha(i), at_next = alpha(j);
    if (dxg && (rc = pde(xt))) return rc;
    if ((rc = net(xt, (float)i, step))) return rc;
    k.xt = xt; k.xt_next = bufs[step & 1];
    k.s0 = sqrtf(a_t); k.s1 = sqrtf(1.0f - a_t); k.sa = sqrtf(at_next);
    k.gw = dxg ? wgt * k.s1 : 0.f;                                        // 5. * (1 - at).sqrt(), fp32 (:1502)
    const DdimNoiseCoefs nc = ddim_noise_coefs(stochastic, sp->eta, a_t, at_next);
    k.c1 = nc.c1; k.c2 = nc.c2;
    if (stochastic) {
      k.noise = rng_seed ? nullptr : eta_noise + (size_t)step * b.total;
      k.seed = reinterpret_cast<const unsigned long long*>(rng_seed); k.draw = (unsigned long long)step;
    } else {
      k.noise = nullptr; k.seed = nullptr;
    }
    const bool store = !return_last || step == S - 1;                   // return_last keeps the last state and x0 only (:1517-1522)
    k.xs = store ? xs_out : nullptr; k.x0s = store ? x0_out : nullptr;
    k.t_xs = return_last ? 0 : step + 1; k.t_x0 = return_last ? 0 : step;
    if ((rc = launch_ddim_cond_step(k, s))) return rc;
    xt = k.xt_next;
  }
  return MCEDM_OK;
}
template <class Net>
static inline int cond_ddim_loop(const mcedm_cond_ddim_desc* sp, const CondDdimLoop& b, const float* init_noise, const float* eta_noise,
                                 const uint64_t* rng_seed, float* xs_out, float* x0_out, int return_last, hipStream_t s, Net&& net) {
  return cond_ddim_loop(sp, b, init_noise, eta_noise, rng_seed, xs_out, x0_out, return_last, s, net, nullptr, 0.f,
                        [](const float*) { return (int)MCEDM_OK; });
}

// What every guided entry of the single-task samplers checks before any launch (with guidance_dx's Darcy grid check)
static inline int guidance_check(const char* who, const mcedm_guidance_desc* gd, int in_channels, const float* cond, int cond_channels,
                                 int H, int W) {
  if (!gd) return MCEDM_OK;
  MCEDM_REQUIRE(gd->system == 1 || gd->system == 2, "%s: gd->system %d: guidance system must be 1 (SWE) or 2 (Darcy)", who, gd->system);
  MCEDM_REQUIRE(in_channels == 1, "%s: gd given to a plan with in_channels %d: PDE guidance is defined for the single-task sampler "
                "(state u, conditioning h in cond[:, 0]), models/ddim.py:1424-1450", who, in_channels);
  MCEDM_REQUIRE(cond != nullptr && cond_channels >= 1, "%s: gd needs cond (h in cond[:, 0]) and sp->cond_channels >= 1 (got cond %s, "
                "cond_channels %d)", who, cond ? "given" : "NULL", cond_channels);
  MCEDM_REQUIRE(gd->system == 1 || (H == W && H > 4), "%s: gd: the Darcy residual needs a square grid larger than 4 x 4 (got %d x %d)",
                who, H, W);
  return MCEDM_OK;
}


// What the dx_cond entries of the epsilon model's samplers check before any launch (mcedm_vp_heun_sample_dxcond,
// mcedm_cond_ddim_sample_dxcond): the plan, the description of the dx residual and the conditioning field it reads
static inline int dxcond_check(const char* who, const mcedm_plan* plan, const mcedm_guidance_desc* dxc, const float* cond,
                               int cond_channels, int H, int W) {
  MCEDM_REQUIRE(plan != nullptr, "%s: null plan", who);
  const mcedm_unet_desc& d = plan->desc;
  MCEDM_REQUIRE(d.dx_mode != MCEDM_DX_NONE && d.in_channels == 1 && d.dx_channels == 1,
                "%s: needs a dx_cond plan of the single-task model (dx_mode %d, in_channels %d, dx_channels %d; state u, one dx "
                "channel), models/ddim.py:1424-1450", who, d.dx_mode, d.in_channels, d.dx_channels);
  MCEDM_REQUIRE(dxc != nullptr, "%s: dxc (the residual whose gradient is the network's dx input) is null", who);
  MCEDM_REQUIRE(dxc->system == 1 || dxc->system == 2, "%s: dxc->system %d: dx system must be 1 (SWE) or 2 (Darcy)", who, dxc->system);
  MCEDM_REQUIRE(cond != nullptr && cond_channels >= 1, "%s: dxc needs cond (h in cond[:, 0]) and sp->cond_channels >= 1 (got cond %s, "
                "cond_channels %d)", who, cond ? "given" : "NULL", cond_channels);
  MCEDM_REQUIRE(dxc->system == 1 || (H == W && H > 4), "%s: dxc: the Darcy residual needs a square grid larger than 4 x 4 (got %d x %d)",
                who, H, W);
  return MCEDM_OK;
}

}  // namespace mcedm
