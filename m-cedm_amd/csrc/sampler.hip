// sampler.hip -- the samplers of the ADM U-Net: the EDM Heun sampler (with mask, PDE guidance and dx_cond), the
// VP-preconditioned Heun sampler of an epsilon network and that network's DDIM sampler.  Host code only: the schedules (fp64) and the order of the launches;
// the loop itself is heun.hpp, the network plan.hip.
#include <algorithm>
#include <cmath>
#include <vector>

#include "heun.hpp"

using namespace mcedm;

// ------------------------------------------------------------------------------------------
// Heun sampler (models/mcedm.py:570-638)
// ------------------------------------------------------------------------------------------
extern "C" int mcedm_edm_t_steps(const mcedm_sampler_desc* sp, double* t) {
  MCEDM_REQUIRE(sp && t, "t_steps: null argument");
  MCEDM_REQUIRE(sp->timesteps >= 2, "t_steps: timesteps=%d (the reference divides by timesteps-1)", sp->timesteps);
  const double smin = std::max(sp->sigma_min, sp->net_sigma_min);   // mcedm.py:579-580
  const double smax = std::min(sp->sigma_max, sp->net_sigma_max);
  const int N = sp->timesteps;
  const double a = std::pow(smax, 1.0 / sp->rho), b = std::pow(smin, 1.0 / sp->rho) - std::pow(smax, 1.0 / sp->rho);
  for (int i = 0; i < N; ++i) t[i] = std::pow(a + (double)i / (double)(N - 1) * b, sp->rho);
  t[N] = 0.0;
  return MCEDM_OK;
}

namespace mcedm {
struct SamplerBufs : HeunBufs { size_t dx, g, dxin; };
static SamplerBufs sampler_bufs(const mcedm_plan& P, int B, int H, int W) {
  const size_t n = (size_t)B * P.desc.in_channels * H * W;
  SamplerBufs s{heun_bufs(n), 0, 0, 0};
  s.dx = heun_take(s, n * 4); s.g = heun_take(s, n * 4);          // PDE guidance: gradient and the Darcy interior scratch
  s.dxin = heun_take(s, n * 4);                                   // dx_cond: the network's dx input
  return s;
}
}  // namespace mcedm

extern "C" int mcedm_sampler_workspace_bytes(const mcedm_plan* plan, int B, int H, int W, size_t* bytes) {
  VariantScope variant_scope__(plan);
  MCEDM_REQUIRE(plan && bytes, "sampler_workspace_bytes: null argument");
  const int rc = mcedm_unet_workspace_bytes(plan, B, H, W, 0, bytes);
  if (rc == MCEDM_OK) *bytes += sampler_bufs(*plan, B, H, W).total;
  return rc;
}

// gd: PDE guidance on the denoised state; dxc: the residual whose gradient at the current state is the network's dx input;
// rng_seed: the churn draws come from the device generator instead of step_noise
static int heun_sample_impl(const mcedm_plan* plan, const void* packed, const mcedm_sampler_desc* sp,
                            const float* cond, const float* mask, const float* init_noise,
                            const double* step_noise, double* out, int return_last, void* workspace,
                            size_t workspace_bytes, int B, int H, int W, const mcedm_guidance_desc* gd, void* stream,
                            const mcedm_guidance_desc* dxc, const uint64_t* rng_seed) {
  MCEDM_REQUIRE(plan && packed && sp && init_noise && out && workspace, "heun_sample: null argument");
  const mcedm_plan& P = *plan;
  int rc;
  MCEDM_REQUIRE(P.desc.in_channels == P.desc.out_channels, "heun_sample: in_channels != out_channels");
  MCEDM_REQUIRE(mask == nullptr || (cond != nullptr && P.desc.cond_channels >= P.desc.in_channels),
                "heun_sample: with a mask, cond must carry hu_known in its first %d channels", P.desc.in_channels);
  MCEDM_REQUIRE(sp->timesteps >= 2 && sp->timesteps <= 4096, "heun_sample: timesteps=%d out of range", sp->timesteps);
  const int N = sp->timesteps;
  std::vector<double> t(N + 1);
  if ((rc = mcedm_edm_t_steps(sp, t.data()))) return rc;
  std::vector<double> gammas(N);
  for (int i = 0; i < N; ++i) {
    const bool in_range = sp->S_min <= t[i] && t[i] <= sp->S_max;                    // mcedm.py:606
    gammas[i] = in_range ? std::min(sp->S_churn / N, std::sqrt(2.0) - 1.0) : 0.0;
    MCEDM_REQUIRE(gammas[i] == 0.0 || step_noise != nullptr || rng_seed != nullptr, "heun_sample: S_churn > 0 needs step_noise (or mcedm_heun_sample_rng)");
  }
  const SamplerBufs sb = sampler_bufs(P, B, H, W);
  AdmNet net;
  if ((rc = adm_bind("heun_sample", P, packed, workspace, workspace_bytes, sb.total, no_extra, B, H, W, 0, 1, stream, &net))) return rc;
  hipStream_t s = net.s;
  HeunState h = heun_state(workspace, sb, B, P.desc.in_channels, (size_t)H * W, N, return_last, out, s);
  const double w = sp->w;
  const float sd = (float)sp->sigma_data;
  float* gscratch = at<float>(workspace, sb.g);
  float* dxin = dxc ? at<float>(workspace, sb.dxin) : nullptr;
  float* dxg = gd ? at<float>(workspace, sb.dx) : nullptr;
  const float wgt = gd ? (float)gd->weight : 0.f;
  // D(x32; sigma), mcedm.py:611-618 / 621-628; dx_cond: dx_in = get_dx_input(h, x32) first (ddim.py:1571, 1584); guidance:
  // its gradient at D afterwards
  auto denoise = [&](double sigma, bool) -> int {
    int e = dxc ? guidance_dx(P.desc.cond_channels, *dxc, cond, h.x32, dxin, gscratch, B, H, W, s) : MCEDM_OK;
    if (e) return e;
    e = denoise_impl(net, h.x32, dxin, cond, nullptr, (float)sigma, w, sd, h.D, nullptr);
    if (e) return e;
    return gd ? guidance_dx(P.desc.cond_channels, *gd, cond, h.D, dxg, gscratch, B, H, W, s) : MCEDM_OK;
  };

  if ((rc = launch_heun_init(cond, P.desc.cond_channels, h.C, h.hw, mask, init_noise, t[0], h.total, h.x, h.x32, s))) return rc;
  if ((rc = heun_store_step(h, 0))) return rc;
  for (int i = 0; i < N; ++i) {
    const double t_cur = t[i], t_next = t[i + 1];
    const double t_hat = t_cur + gammas[i] * t_cur;                                   // mcedm.py:607
    if (gammas[i] != 0.0) {
      const double c = std::sqrt(t_hat * t_hat - t_cur * t_cur) * sp->S_noise;
      if ((rc = heun_churn(h, c, step_noise ? step_noise + (size_t)i * h.total : nullptr,
                           reinterpret_cast<const unsigned long long*>(rng_seed), (unsigned long long)i, mask))) return rc;
    }
    if ((rc = heun_update(h, i, t_hat, t_next, mask, denoise, dxg, wgt, (float)t_hat))) return rc;
    if ((rc = heun_store_step(h, i + 1))) return rc;
  }
  return heun_store_last(h);
}

extern "C" int mcedm_heun_sample(const mcedm_plan* plan, const void* packed, const mcedm_sampler_desc* sp,
                                 const float* cond, const float* mask, const float* init_noise,
                                 const double* step_noise, double* out, int return_last, void* workspace,
                                 size_t workspace_bytes, int B, int H, int W, void* stream) {
  VariantScope variant_scope__(plan);
  return heun_sample_impl(plan, packed, sp, cond, mask, init_noise, step_noise, out, return_last, workspace, workspace_bytes,
                          B, H, W, nullptr, stream, nullptr, nullptr);
}

// The churn noise of every step generated inside the kernel that applies it (Philox4x32-10 keyed by *rng_seed, draw = step
// index): no [timesteps][B][C][H][W] fp64 tensor (2.1 GB at 50 x 160 x 2 x 128 x 128, the reference's shipped sampler config,
// configs/diff_sampler/edm_sampler.yaml) and one HIP graph replays with fresh noise after the host bumps the seed.
extern "C" int mcedm_heun_sample_rng(const mcedm_plan* plan, const void* packed, const mcedm_sampler_desc* sp,
                                     const float* cond, const float* mask, const float* init_noise, const uint64_t* rng_seed,
                                     double* out, int return_last, void* workspace, size_t workspace_bytes, int B, int H, int W,
                                     void* stream) {
  VariantScope variant_scope__(plan);
  MCEDM_REQUIRE(rng_seed != nullptr, "heun_sample_rng: rng_seed (a 64-bit seed in device memory) is null");
  return heun_sample_impl(plan, packed, sp, cond, mask, init_noise, nullptr, out, return_last, workspace, workspace_bytes,
                          B, H, W, nullptr, stream, nullptr, rng_seed);
}

// the two PDE entries, each with its draws read from step_noise or generated from rng_seed (at most one of them non-NULL)
static int heun_guided(const mcedm_plan* plan, const void* packed, const mcedm_sampler_desc* sp, const mcedm_guidance_desc* gd,
                       const float* cond, const float* mask, const float* init_noise, const double* step_noise,
                       const uint64_t* rng_seed, double* out, int return_last, void* workspace, size_t workspace_bytes, int B, int H,
                       int W, void* stream) {
  MCEDM_REQUIRE(gd != nullptr && (gd->system == 1 || gd->system == 2), "heun_sample_guided: guidance system must be 1 (SWE) or 2 (Darcy)");
  MCEDM_REQUIRE(plan && plan->desc.in_channels == 1 && plan->desc.cond_channels >= 1 && cond != nullptr && mask == nullptr,
                "heun_sample_guided: PDE guidance is defined for the single-task sampler (state u, conditioning h in cond[:, 0]; "
                "mask NULL), models/ddim.py:1532-1601; the joint model's hook fails in the reference (models/mcedm.py:500-518)");
  return heun_sample_impl(plan, packed, sp, cond, mask, init_noise, step_noise, out, return_last, workspace, workspace_bytes,
                          B, H, W, gd, stream, nullptr, rng_seed);
}

extern "C" int mcedm_heun_sample_guided(const mcedm_plan* plan, const void* packed, const mcedm_sampler_desc* sp,
                                        const mcedm_guidance_desc* gd, const float* cond, const float* mask,
                                        const float* init_noise, const double* step_noise, double* out, int return_last,
                                        void* workspace, size_t workspace_bytes, int B, int H, int W, void* stream) {
  VariantScope variant_scope__(plan);
  return heun_guided(plan, packed, sp, gd, cond, mask, init_noise, step_noise, nullptr, out, return_last, workspace, workspace_bytes, B,
                     H, W, stream);
}

extern "C" int mcedm_heun_sample_guided_rng(const mcedm_plan* plan, const void* packed, const mcedm_sampler_desc* sp,
                                            const mcedm_guidance_desc* gd, const float* cond, const float* mask,
                                            const float* init_noise, const uint64_t* rng_seed, double* out, int return_last,
                                            void* workspace, size_t workspace_bytes, int B, int H, int W, void* stream) {
  VariantScope variant_scope__(plan);
  MCEDM_REQUIRE(rng_seed != nullptr, "heun_sample_guided_rng: rng_seed (a 64-bit seed in device memory) is null");
  return heun_guided(plan, packed, sp, gd, cond, mask, init_noise, nullptr, rng_seed, out, return_last, workspace, workspace_bytes, B,
                     H, W, stream);
}

static int heun_dxcond(const mcedm_plan* plan, const void* packed, const mcedm_sampler_desc* sp, const mcedm_guidance_desc* dxc,
                       const mcedm_guidance_desc* gd, const float* cond, const float* init_noise, const double* step_noise,
                       const uint64_t* rng_seed, double* out, int return_last, void* workspace, size_t workspace_bytes, int B, int H,
                       int W, void* stream) {
  MCEDM_REQUIRE(dxc != nullptr && (dxc->system == 1 || dxc->system == 2), "heun_sample_dxcond: dx system must be 1 (SWE) or 2 (Darcy)");
  MCEDM_REQUIRE(gd == nullptr || gd->system == 1 || gd->system == 2, "heun_sample_dxcond: guidance system must be 1 (SWE) or 2 (Darcy)");
  MCEDM_REQUIRE(plan && plan->desc.dx_mode != MCEDM_DX_NONE && plan->desc.dx_channels == 1 && plan->desc.in_channels == 1 &&
                    plan->desc.cond_channels >= 1 && cond != nullptr,
                "heun_sample_dxcond: needs a dx_cond plan of the single-task model (state u, conditioning h in cond[:, 0], one dx "
                "channel), models/ddim.py:1424-1450, 1532-1601");
  return heun_sample_impl(plan, packed, sp, cond, nullptr, init_noise, step_noise, out, return_last, workspace, workspace_bytes,
                          B, H, W, gd, stream, dxc, rng_seed);
}

extern "C" int mcedm_heun_sample_dxcond(const mcedm_plan* plan, const void* packed, const mcedm_sampler_desc* sp,
                                        const mcedm_guidance_desc* dxc, const mcedm_guidance_desc* gd, const float* cond,
                                        const float* init_noise, const double* step_noise, double* out, int return_last,
                                        void* workspace, size_t workspace_bytes, int B, int H, int W, void* stream) {
  VariantScope variant_scope__(plan);
  return heun_dxcond(plan, packed, sp, dxc, gd, cond, init_noise, step_noise, nullptr, out, return_last, workspace, workspace_bytes, B,
                     H, W, stream);
}

extern "C" int mcedm_heun_sample_dxcond_rng(const mcedm_plan* plan, const void* packed, const mcedm_sampler_desc* sp,
                                            const mcedm_guidance_desc* dxc, const mcedm_guidance_desc* gd, const float* cond,
                                            const float* init_noise, const uint64_t* rng_seed, double* out, int return_last,
                                            void* workspace, size_t workspace_bytes, int B, int H, int W, void* stream) {
  VariantScope variant_scope__(plan);
  MCEDM_REQUIRE(rng_seed != nullptr, "heun_sample_dxcond_rng: rng_seed (a 64-bit seed in device memory) is null");
  return heun_dxcond(plan, packed, sp, dxc, gd, cond, init_noise, nullptr, rng_seed, out, return_last, workspace, workspace_bytes, B,
                     H, W, stream);
}

// ------------------------------------------------------------------------------------------
// VP-preconditioned Heun sampler of an epsilon network (PlCondDdim.sample_edm, models/ddim.py:1532-1601)
// ------------------------------------------------------------------------------------------
namespace mcedm {
struct VpBufs : HeunBufs { size_t condp, dx, g, dxin; };
static VpBufs vp_bufs(const mcedm_plan& P, int B, int H, int W, bool pde = false, bool dxc = false) {
  const size_t n = (size_t)B * P.desc.in_channels * H * W;
  VpBufs v{heun_bufs(n), 0, 0, 0, 0};
  // cond' = cat(cond, zeros) of a self-conditioning plan
  v.condp = heun_take(v, (size_t)B * P.desc.cond_channels * H * W * 4);
  if (pde) { v.dx = heun_take(v, n * 4); v.g = heun_take(v, n * 4); }      // PDE guidance: gradient, Darcy scratch
  // dx_cond: the network's dx input, a buffer of its own; the Darcy scratch serves both (the launches are serial on one stream)
  if (dxc) { v.dxin = heun_take(v, n * 4); if (!pde) v.g = heun_take(v, n * 4); }
  return v;
}

// c_in = 1 / (sigma ** 2 + 1).sqrt() with sigma = t.to(torch.float32), fp32 (:917-921)
static inline float vp_c_in(double sigma_d) {
  const float sigma = (float)sigma_d;
  return 1.0f / sqrtf(sigma * sigma + 1.0f);
}

// get_denoised (models/ddim.py:915-947) at one noise level: D = x + (-sigma) F(c_in cat(cond', x), c_noise).  dx (dx_cond
// plans): fl(c_in * get_dx_input(h, x)) (:933-934), scaled where it was stored, so a cat_dx plan's dx rows of conv_in are 1
static int vp_denoise(const AdmNet& net, const float* x32, const float* condp, const float* dx, double sigma_d, float c_noise,
                      double w, float* D) {
  const mcedm_unet_desc& d = net.plan->desc;
  int rc;
  const float sigma = (float)sigma_d;                                   // t.to(torch.float32)
  const float c_in = vp_c_in(sigma_d);
  if ((rc = launch_vp_prepare(c_in, d.cond_channels + d.in_channels, c_noise, net.coef_in(), net.c_noise(), net.s,
                              d.dx_mode == MCEDM_DX_CAT ? d.dx_channels : 0))) return rc;
  // :938-942, taken when cond OR dx is given; the second evaluation drops both
  float* Fu = std::fabs(w) >= 0.001 && (condp != nullptr || dx != nullptr) ? net.Fu() : nullptr;
  if ((rc = net.forward_cfg(AdmIn{x32, dx, condp, net.coef_in(), net.c_noise()}, net.F(), Fu))) return rc;
  return launch_vp_cfg_finish(x32, net.F(), Fu, w, sigma, (size_t)net.B * d.out_channels * net.H * net.W, D, net.s);
}
}  // namespace mcedm

extern "C" int mcedm_vp_sampler_workspace_bytes(const mcedm_plan* plan, int B, int H, int W, size_t* bytes) {
  VariantScope variant_scope__(plan);
  MCEDM_REQUIRE(plan && bytes, "vp_sampler_workspace_bytes: null argument");
  const int rc = mcedm_unet_workspace_bytes(plan, B, H, W, 0, bytes);
  if (rc == MCEDM_OK) *bytes += vp_bufs(*plan, B, H, W).total;
  return rc;
}

// gd: PDE guidance, dx = get_dx_log_prob(h, D) after every get_denoised (:1576, 1589), h = plane 0 of the caller's cond
// dxc (the _dxcond entry, whose checks dxcond_check has made): dx_in = get_dx_input(h, x) in front of every get_denoised
// (:1571, 1584), evaluated on the unscaled h.x32 and stored as fl(c_in * dx_in)
static int vp_sample_impl(const mcedm_plan* plan, const void* packed, const mcedm_vp_sampler_desc* sp, const mcedm_guidance_desc* gd,
                          const float* cond, const float* init_noise, const double* step_noise, const uint64_t* rng_seed, double* out,
                          int return_last, void* workspace, size_t workspace_bytes, int B, int H, int W, void* stream,
                          const mcedm_guidance_desc* dxc = nullptr) {
  MCEDM_REQUIRE(plan && packed && sp && init_noise && out && workspace, "vp_heun_sample: null argument");
  MCEDM_REQUIRE(!(step_noise && rng_seed), "vp_heun_sample: step_noise and rng_seed are both given (at most one of them)");
  MCEDM_REQUIRE(sp->t_steps && sp->t_hat && sp->c_noise, "vp_heun_sample: null schedule array");
  const mcedm_plan& P = *plan;
  int rc;
  MCEDM_REQUIRE(P.desc.in_channels == P.desc.out_channels, "vp_heun_sample: in_channels != out_channels");
  MCEDM_REQUIRE(dxc != nullptr || P.desc.dx_mode == MCEDM_DX_NONE, "vp_heun_sample: dx_cond plans are not supported");
  MCEDM_REQUIRE(sp->cond_channels >= 0 && sp->cond_channels <= P.desc.cond_channels,
                "vp_heun_sample: cond_channels %d outside [0, %d]", sp->cond_channels, P.desc.cond_channels);
  MCEDM_REQUIRE(cond == nullptr || sp->cond_channels > 0, "vp_heun_sample: cond given with cond_channels 0");
  if ((rc = guidance_check("vp_heun_sample", gd, P.desc.in_channels, cond, sp->cond_channels, H, W))) return rc;
  if ((rc = vp_check_schedule(sp, step_noise, rng_seed))) return rc;
  const int N = sp->timesteps;
  const VpBufs vb = vp_bufs(P, B, H, W, gd != nullptr, dxc != nullptr);
  AdmNet net;
  if ((rc = adm_bind("vp_heun_sample", P, packed, workspace, workspace_bytes, vb.total, no_extra, B, H, W, 0, 1, stream, &net))) return rc;
  HeunState h = heun_state(workspace, vb, B, P.desc.in_channels, (size_t)H * W, N, return_last, out, net.s);
  // cond' once per call: cond in its channels, zeros in the self-conditioning ones (get_self_cond_edm returns None)
  const float* condp = cond;
  if (cond && sp->cond_channels < P.desc.cond_channels) {
    float* st = at<float>(workspace, vb.condp);
    if ((rc = mcedm_eps_self_cond(nullptr, nullptr, nullptr, nullptr, nullptr, 0, cond, sp->cond_channels,
                                  P.desc.cond_channels - sp->cond_channels, B, H, W, st, stream))) return rc;
    condp = st;
  }
  float* dxg = gd ? at<float>(workspace, vb.dx) : nullptr;
  float* gscratch = gd || dxc ? at<float>(workspace, vb.g) : nullptr;
  float* dxin = dxc ? at<float>(workspace, vb.dxin) : nullptr;
  // the guidance and dx_cond read the caller's cond [B, sp->cond_channels, H, W], not cond'
  return vp_heun_loop(h, sp, init_noise, step_noise, rng_seed, [&](double sigma, float c_noise) -> int {
    int e = dxc ? guidance_dx(sp->cond_channels, *dxc, cond, h.x32, dxin, gscratch, B, H, W, net.s, vp_c_in(sigma)) : MCEDM_OK;
    if (e) return e;
    e = vp_denoise(net, h.x32, condp, dxin, sigma, c_noise, sp->w, h.D);
    if (e || !gd) return e;
    return guidance_dx(sp->cond_channels, *gd, cond, h.D, dxg, gscratch, B, H, W, net.s);
  }, dxg, gd ? (float)gd->weight : 0.f);
}

extern "C" int mcedm_vp_heun_sample(const mcedm_plan* plan, const void* packed, const mcedm_vp_sampler_desc* sp, const float* cond,
                                    const float* init_noise, const double* step_noise, double* out, int return_last,
                                    void* workspace, size_t workspace_bytes, int B, int H, int W, void* stream) {
  VariantScope variant_scope__(plan);
  return vp_sample_impl(plan, packed, sp, nullptr, cond, init_noise, step_noise, nullptr, out, return_last, workspace, workspace_bytes,
                        B, H, W, stream);
}

extern "C" int mcedm_vp_heun_sample_rng(const mcedm_plan* plan, const void* packed, const mcedm_vp_sampler_desc* sp,
                                        const float* cond, const float* init_noise, const uint64_t* rng_seed, double* out,
                                        int return_last, void* workspace, size_t workspace_bytes, int B, int H, int W,
                                        void* stream) {
  VariantScope variant_scope__(plan);
  MCEDM_REQUIRE(rng_seed != nullptr, "vp_heun_sample_rng: rng_seed (a 64-bit seed in device memory) is null");
  return vp_sample_impl(plan, packed, sp, nullptr, cond, init_noise, nullptr, rng_seed, out, return_last, workspace, workspace_bytes,
                        B, H, W, stream);
}

extern "C" int mcedm_vp_guided_workspace_bytes(const mcedm_plan* plan, int B, int H, int W, size_t* bytes) {
  VariantScope variant_scope__(plan);
  MCEDM_REQUIRE(plan && bytes, "vp_guided_workspace_bytes: null argument");
  AdmNet net;                            // one noise label for the whole batch, as the sampler lays its forward out: exact
  const int rc = adm_sizes(*plan, B, H, W, 0, 1, &net, bytes);
  if (rc == MCEDM_OK) *bytes += vp_bufs(*plan, B, H, W, true).total;
  return rc;
}

extern "C" int mcedm_vp_heun_sample_guided(const mcedm_plan* plan, const void* packed, const mcedm_vp_sampler_desc* sp,
                                           const mcedm_guidance_desc* gd, const float* cond, const float* init_noise,
                                           const double* step_noise, const uint64_t* rng_seed, double* out, int return_last,
                                           void* workspace, size_t workspace_bytes, int B, int H, int W, void* stream) {
  VariantScope variant_scope__(plan);
  return vp_sample_impl(plan, packed, sp, gd, cond, init_noise, step_noise, rng_seed, out, return_last, workspace, workspace_bytes, B,
                        H, W, stream);
}

extern "C" int mcedm_vp_dxcond_workspace_bytes(const mcedm_plan* plan, int B, int H, int W, size_t* bytes) {
  VariantScope variant_scope__(plan);
  MCEDM_REQUIRE(plan && bytes, "vp_dxcond_workspace_bytes: null argument");
  AdmNet net;                            // exact, like the guided query; sized for dxc AND gd
  const int rc = adm_sizes(*plan, B, H, W, 0, 1, &net, bytes);
  if (rc == MCEDM_OK) *bytes += vp_bufs(*plan, B, H, W, true, true).total;
  return rc;
}

extern "C" int mcedm_vp_heun_sample_dxcond(const mcedm_plan* plan, const void* packed, const mcedm_vp_sampler_desc* sp,
                                           const mcedm_guidance_desc* dxc, const mcedm_guidance_desc* gd, const float* cond,
                                           const float* init_noise, const double* step_noise, const uint64_t* rng_seed, double* out,
                                           int return_last, void* workspace, size_t workspace_bytes, int B, int H, int W,
                                           void* stream) {
  VariantScope variant_scope__(plan);
  MCEDM_REQUIRE(sp != nullptr, "vp_heun_sample_dxcond: null argument");
  const int rc = dxcond_check("vp_heun_sample_dxcond", plan, dxc, cond, sp->cond_channels, H, W);
  return rc ? rc : vp_sample_impl(plan, packed, sp, gd, cond, init_noise, step_noise, rng_seed, out, return_last, workspace,
                                  workspace_bytes, B, H, W, stream, dxc);
}

// ------------------------------------------------------------------------------------------
// DDIM sampler of the conditional epsilon network (PlCondDdim.sample, models/ddim.py:1452-1530): fp32 throughout
// ------------------------------------------------------------------------------------------
namespace mcedm {
// the sampler's own buffers in front of the network's workspace, each 256-byte aligned
struct CondDdimBufs { size_t xt, xtn, F, Fu, condp, condu, total, dx, g, dxin; };
static CondDdimBufs cond_ddim_bufs(const mcedm_plan& P, int B, int H, int W, bool pde = false, bool dxc = false) {
  CondDdimBufs b{};
  const size_t hw = (size_t)H * W, n = (size_t)B * P.desc.in_channels * hw;
  b.xt = heun_take(b, n * 4); b.xtn = heun_take(b, n * 4);
  b.F = heun_take(b, (size_t)B * P.desc.out_channels * hw * 4); b.Fu = heun_take(b, (size_t)B * P.desc.out_channels * hw * 4);
  // cond' = cat(cond, x0_t) and cat(0, x0_t), what the unconditional pass reads
  b.condp = heun_take(b, (size_t)B * P.desc.cond_channels * hw * 4); b.condu = heun_take(b, (size_t)B * P.desc.cond_channels * hw * 4);
  if (pde) { b.dx = heun_take(b, n * 4); b.g = heun_take(b, n * 4); }      // PDE guidance: gradient, Darcy scratch
  if (dxc) { b.dxin = heun_take(b, n * 4); if (!pde) b.g = heun_take(b, n * 4); }      // dx_cond: the network's dx input (as in vp_bufs)
  return b;
}
}  // namespace mcedm

extern "C" int mcedm_cond_ddim_workspace_bytes(const mcedm_plan* plan, int B, int H, int W, size_t* bytes) {
  VariantScope variant_scope__(plan);
  MCEDM_REQUIRE(plan && bytes, "cond_ddim_workspace_bytes: null argument");
  AdmNet net;                            // one noise label for the whole batch, as the sampler lays its forward out
  const int rc = adm_sizes(*plan, B, H, W, 0, 1, &net, bytes);
  if (rc == MCEDM_OK) *bytes += cond_ddim_bufs(*plan, B, H, W).total;
  return rc;
}

// eta_noise / rng_seed: the uniform draws of the stochastic steps, read from slice k or generated in the step kernel as draw k
// gd: PDE guidance, dx = get_dx_log_prob(h, xt) at every step's noisy state (:1501), h = plane 0 of the caller's cond
// dxc (the _dxcond entry, whose checks dxcond_check has made): dx_in = get_dx_input(h, xt) at the same state (:1492), unscaled,
// the network's dx input of the conditional pass
static int cond_ddim_impl(const mcedm_plan* plan, const void* packed, const mcedm_cond_ddim_desc* sp, const mcedm_guidance_desc* gd,
                          const float* cond, const float* init_noise, const float* eta_noise, const uint64_t* rng_seed, float* xs_out,
                          float* x0_out, int return_last, void* workspace, size_t workspace_bytes, int B, int H, int W, void* stream,
                          const mcedm_guidance_desc* dxc = nullptr) {
  MCEDM_REQUIRE(plan && packed && sp && init_noise && xs_out && x0_out && workspace, "cond_ddim_sample: null argument");
  MCEDM_REQUIRE(!(eta_noise && rng_seed), "cond_ddim_sample: eta_noise and rng_seed are both given (at most one of them)");
  const mcedm_plan& P = *plan;
  int rc;
  MCEDM_REQUIRE(P.desc.in_channels == P.desc.out_channels, "cond_ddim_sample: in_channels != out_channels");
  MCEDM_REQUIRE(dxc != nullptr || P.desc.dx_mode == MCEDM_DX_NONE, "cond_ddim_sample: dx_cond plans are not supported");
  const int C = P.desc.in_channels, Cp = P.desc.cond_channels, cc = sp->cond_channels;
  MCEDM_REQUIRE(cc >= 0 && cc <= Cp, "cond_ddim_sample: cond_channels %d outside [0, %d]", cc, Cp);
  MCEDM_REQUIRE((cond != nullptr) == (cc > 0), "cond_ddim_sample: cond goes with cond_channels > 0 (and only with it)");
  MCEDM_REQUIRE(!sp->self_cond || cc + C <= Cp,
                "cond_ddim_sample: self-conditioning asked of a plan whose conditioning input is not widened (%d + %d > %d channels)",
                cc, C, Cp);
  if ((rc = guidance_check("cond_ddim_sample", gd, C, cond, cc, H, W))) return rc;
  if ((rc = cond_ddim_check_schedule(sp, eta_noise, rng_seed))) return rc;
  const bool guided = cond_ddim_guided(sp);
  const CondDdimBufs cb = cond_ddim_bufs(P, B, H, W, gd != nullptr, dxc != nullptr);
  AdmNet net;
  if ((rc = adm_bind("cond_ddim_sample", P, packed, workspace, workspace_bytes, cb.total, no_extra, B, H, W, 0, 1, stream, &net))) return rc;
  const size_t hw = (size_t)H * W, total = (size_t)B * C * hw;
  hipStream_t s = net.s;
  // cond' once per call: cond in its channels, zeros in the others (x_self_cond is None in the first step); the step kernel
  // keeps the self-conditioning channels current from then on.  Guided: the twin with zeros for cond as well.
  float* condp = Cp > 0 ? at<float>(workspace, cb.condp) : nullptr;
  float* condu = Cp > 0 && guided ? at<float>(workspace, cb.condu) : nullptr;
  if (condp && (rc = mcedm_eps_self_cond(nullptr, nullptr, nullptr, nullptr, nullptr, 0, cond, cc, Cp - cc, B, H, W, condp, stream)))
    return rc;
  if (condu && (rc = mcedm_eps_self_cond(nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, cc, Cp - cc, B, H, W, condu, stream)))
    return rc;
  CondDdimLoop lp{C, hw, total, at<float>(workspace, cb.xt), at<float>(workspace, cb.xtn), at<float>(workspace, cb.F),
                  guided ? at<float>(workspace, cb.Fu) : nullptr, sp->self_cond ? condp : nullptr, sp->self_cond ? condu : nullptr, Cp, cc};
  float* dxg = gd ? at<float>(workspace, cb.dx) : nullptr;
  float* gscratch = gd || dxc ? at<float>(workspace, cb.g) : nullptr;
  float* dxin = dxc ? at<float>(workspace, cb.dxin) : nullptr;
  const int dxrows = P.desc.dx_mode == MCEDM_DX_CAT ? P.desc.dx_channels : 0;
  // the network sees xt itself (no c_in on this path: conv_in rows scaled by 1) under the label t
  return cond_ddim_loop(sp, lp, init_noise, eta_noise, rng_seed, xs_out, x0_out, return_last, s, [&](const float* xt, float t, int) -> int {
    int e;
    // dx_cond: the residual gradient at the step's own xt, in front of the step's network launches
    if (dxc && (e = guidance_dx(cc, *dxc, cond, xt, dxin, gscratch, B, H, W, s))) return e;
    if ((e = launch_vp_prepare(1.0f, Cp + C + dxrows, t, net.coef_in(), net.c_noise(), s))) return e;
    AdmIn in{xt, dxin, condp, net.coef_in(), net.c_noise()};
    if ((e = net.forward(in, lp.F)) || !guided) return e;
    in.cond = condu; in.dx = nullptr; // (not forward_cfg: the twin keeps the self-conditioning channels; cond is zeros, dx None)
    return net.forward(in, lp.Fu);
  }, dxg, gd ? (float)gd->weight : 0.f, [&](const float* xt) -> int {
    return guidance_dx(cc, *gd, cond, xt, dxg, gscratch, B, H, W, s);      // the caller's cond [B, cc, H, W], not cond'
  });
}

extern "C" int mcedm_cond_ddim_sample(const mcedm_plan* plan, const void* packed, const mcedm_cond_ddim_desc* sp, const float* cond,
                                      const float* init_noise, const float* eta_noise, float* xs_out, float* x0_out,
                                      int return_last, void* workspace, size_t workspace_bytes, int B, int H, int W,
                                      void* stream) {
  VariantScope variant_scope__(plan);
  return cond_ddim_impl(plan, packed, sp, nullptr, cond, init_noise, eta_noise, nullptr, xs_out, x0_out, return_last, workspace,
                        workspace_bytes, B, H, W, stream);
}

extern "C" int mcedm_cond_ddim_sample_rng(const mcedm_plan* plan, const void* packed, const mcedm_cond_ddim_desc* sp,
                                          const float* cond, const float* init_noise, const uint64_t* rng_seed, float* xs_out,
                                          float* x0_out, int return_last, void* workspace, size_t workspace_bytes, int B, int H,
                                          int W, void* stream) {
  VariantScope variant_scope__(plan);
  MCEDM_REQUIRE(rng_seed != nullptr, "cond_ddim_sample_rng: rng_seed (a 64-bit seed in device memory) is null");
  return cond_ddim_impl(plan, packed, sp, nullptr, cond, init_noise, nullptr, rng_seed, xs_out, x0_out, return_last, workspace,
                        workspace_bytes, B, H, W, stream);
}

extern "C" int mcedm_cond_ddim_guided_workspace_bytes(const mcedm_plan* plan, int B, int H, int W, size_t* bytes) {
  VariantScope variant_scope__(plan);
  MCEDM_REQUIRE(plan && bytes, "cond_ddim_guided_workspace_bytes: null argument");
  AdmNet net;
  const int rc = adm_sizes(*plan, B, H, W, 0, 1, &net, bytes);
  if (rc == MCEDM_OK) *bytes += cond_ddim_bufs(*plan, B, H, W, true).total;
  return rc;
}

extern "C" int mcedm_cond_ddim_sample_guided(const mcedm_plan* plan, const void* packed, const mcedm_cond_ddim_desc* sp,
                                             const mcedm_guidance_desc* gd, const float* cond, const float* init_noise,
                                             const float* eta_noise, const uint64_t* rng_seed, float* xs_out, float* x0_out,
                                             int return_last, void* workspace, size_t workspace_bytes, int B, int H, int W,
                                             void* stream) {
  VariantScope variant_scope__(plan);
  return cond_ddim_impl(plan, packed, sp, gd, cond, init_noise, eta_noise, rng_seed, xs_out, x0_out, return_last, workspace,
                        workspace_bytes, B, H, W, stream);
}

extern "C" int mcedm_cond_ddim_dxcond_workspace_bytes(const mcedm_plan* plan, int B, int H, int W, size_t* bytes) {
  VariantScope variant_scope__(plan);
  MCEDM_REQUIRE(plan && bytes, "cond_ddim_dxcond_workspace_bytes: null argument");
  AdmNet net;                            // sized for dxc AND gd
  const int rc = adm_sizes(*plan, B, H, W, 0, 1, &net, bytes);
  if (rc == MCEDM_OK) *bytes += cond_ddim_bufs(*plan, B, H, W, true, true).total;
  return rc;
}

extern "C" int mcedm_cond_ddim_sample_dxcond(const mcedm_plan* plan, const void* packed, const mcedm_cond_ddim_desc* sp,
                                             const mcedm_guidance_desc* dxc, const mcedm_guidance_desc* gd, const float* cond,
                                             const float* init_noise, const float* eta_noise, const uint64_t* rng_seed,
                                             float* xs_out, float* x0_out, int return_last, void* workspace, size_t workspace_bytes,
                                             int B, int H, int W, void* stream) {
  VariantScope variant_scope__(plan);
  MCEDM_REQUIRE(sp != nullptr, "cond_ddim_sample_dxcond: null argument");
  const int rc = dxcond_check("cond_ddim_sample_dxcond", plan, dxc, cond, sp->cond_channels, H, W);
  return rc ? rc : cond_ddim_impl(plan, packed, sp, gd, cond, init_noise, eta_noise, rng_seed, xs_out, x0_out, return_last,
                                  workspace, workspace_bytes, B, H, W, stream, dxc);
}
