// edm.hip -- K7 (EDM preconditioning), K8 (Heun sampler state updates, fp64), K9 (masked EDM
// loss + its gradient), K11 (grad-clip + Adam + EMA).  All HBM-bound elementwise / reduction
// kernels: one pass over the tensors, coalesced, grid-stride.
//
// The fp64 sampler arithmetic mirrors the evaluation order of models/mcedm.py:594-628 term by
// term, so this file is compiled with -ffp-contract=off (see build.py).
#include "common.hpp"
#include "edm.hpp"
#include "prof.hpp"

namespace mcedm {

static inline int grid_for(size_t n) {
  size_t b = (n + 255) / 256;
  return (int)(b < 2048 ? (b ? b : 1) : 2048);
}

// ---- K7a: per-sample EDM coefficients (mcedm.py:203-206 / 448-451), fp32 like the reference.
// Writes c_skip/c_out/c_in/c_noise rows and the conv_in transform table: cond channels pass
// through, state channels are scaled by c_in (mcedm.py:208: only x is scaled, not cond).
__global__ void precond_prepare_kernel(const float* __restrict__ sigma_dev, float sigma_host, int use_host, int n,
                                       float sigma_data, int cond_ch, int in_ch, int dx_ch, float* __restrict__ coefs4,
                                       float* __restrict__ c_noise, Coef* __restrict__ conv_in_coef) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float s = use_host ? sigma_host : sigma_dev[i];
  const float sd2 = sigma_data * sigma_data;
  const float s2 = s * s;
  const float c_skip = sd2 / (s2 + sd2);
  const float c_out = s * sigma_data / sqrtf(s2 + sd2);
  const float c_in = 1.0f / sqrtf(sd2 + s2);
  const float cn = logf(s) / 4.0f;
  coefs4[4 * i + 0] = c_skip;
  coefs4[4 * i + 1] = c_out;
  coefs4[4 * i + 2] = c_in;
  coefs4[4 * i + 3] = cn;
  c_noise[i] = cn;
  // rows of cat(cond, x, dx): only x is scaled by c_in (adm_blocks.py:319-340 is handed c_in * x, mcedm.py:208)
  const int Ct = cond_ch + in_ch + dx_ch;
  for (int c = 0; c < Ct; ++c)
    conv_in_coef[(size_t)i * Ct + c] = Coef{0.f, (c < cond_ch || c >= cond_ch + in_ch) ? 1.0f : c_in, 0.f, 0.f};
}

int launch_precond_prepare(const float* sigma_dev, float sigma_host, int use_host, int n, float sigma_data,
                           int cond_ch, int in_ch, int dx_ch, float* coefs4, float* c_noise, Coef* conv_in_coef,
                           hipStream_t stream) {
  hipLaunchKernelGGL(precond_prepare_kernel, dim3(ceil_div(n, 64)), dim3(64), 0, stream, sigma_dev, sigma_host,
                     use_host, n, sigma_data, cond_ch, in_ch, dx_ch, coefs4, c_noise, conv_in_coef);
  MCEDM_LAUNCH_CHECK("precond_prepare_kernel");
  return MCEDM_OK;
}

// ---- K7b: D = c_skip*x + c_out*F  (mcedm.py:210 / 460); optional classifier-free blend
// F = (w+1)*F - w*F_uncond first (mcedm.py:457-458), w1 = fl32(w + 1) with the sum formed in double like the reference's
// Python scalar (fl32(fl32(w) + 1) is another number for one w in eight).
__global__ void precond_finish_kernel(const float* __restrict__ x, const float* __restrict__ F,
                                      const float* __restrict__ Fu, float w1, float w, const float* __restrict__ coefs4,
                                      int n_sigma, size_t per_sample, size_t total, float* __restrict__ D,
                                      float* __restrict__ F_out) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const size_t b = n_sigma == 1 ? 0 : i / per_sample;
    float f = F[i];
    if (Fu) f = w1 * f - w * Fu[i];
    if (F_out) F_out[i] = f;
    D[i] = coefs4[4 * b] * x[i] + coefs4[4 * b + 1] * f;
  }
}

int launch_precond_finish(const float* x, const float* F, const float* Fu, double w, const float* coefs4, int n_sigma,
                          size_t per_sample, size_t total, float* D, float* F_out, hipStream_t stream) {
  hipLaunchKernelGGL(precond_finish_kernel, dim3(grid_for(total)), dim3(256), 0, stream, x, F, Fu, (float)(w + 1.0), (float)w, coefs4, n_sigma,
                     per_sample, total, D, F_out);
  MCEDM_LAUNCH_CHECK("precond_finish_kernel");
  return MCEDM_OK;
}

// ---- K8: sampler state (fp64) ---------------------------------------------------------------
// x0 = hu_known*(1-mask) + (noise*t0)*mask                      (mcedm.py:594-597)
__global__ void heun_init_kernel(const float* __restrict__ cond, int cond_ch, int in_ch, size_t hw,
                                 const float* __restrict__ mask, const float* __restrict__ noise, double t0,
                                 size_t total, double* __restrict__ x, float* __restrict__ x32) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const size_t b = i / (in_ch * hw), r = i % (in_ch * hw);
    // mask == NULL: the unmasked sampler of PlCondEdm (models/ddim.py:1556): x0 = noise * t0 (0 + v and v * 1 are exact)
    const float m = mask ? mask[i] : 1.0f;
    const float known = mask ? cond[b * cond_ch * hw + r] : 0.0f;          // cond[:, 0:in_ch]
    const float keep = known * (1.0f - m);                   // fp32 product like the reference
    const double v = (double)keep + ((double)noise[i] * t0) * (double)m;
    x[i] = v;
    x32[i] = (float)v;
  }
}

// x_hat = x_cur + (c*eps)*mask, c = sqrt(t_hat^2 - t_cur^2)*S_noise   (mcedm.py:608)
__global__ void heun_churn_kernel(double* __restrict__ x, const double* __restrict__ eps, const float* __restrict__ mask,
                                  double c, size_t total, float* __restrict__ x32) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const double v = x[i] + (c * eps[i]) * (mask ? (double)mask[i] : 1.0);
    x[i] = v;
    x32[i] = (float)v;
  }
}

// d = (x_hat - D)/t_hat ; x_next = x_hat + ((t_next - t_hat)*d)*mask    (mcedm.py:617-618)
// dxg != NULL: PDE guidance of the single-task sampler, d = (x_hat - D)/t_hat - weight * dx / t_hat with the guidance
// term formed in fp32 (models/ddim.py:1577-1579)
__global__ void heun_euler_kernel(const double* __restrict__ x_hat, const float* __restrict__ D,
                                  const float* __restrict__ mask, double t_hat, double dt, size_t total,
                                  double* __restrict__ d_cur, double* __restrict__ x_next, float* __restrict__ x32,
                                  const float* __restrict__ dxg, float wgt, float gdiv) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const double xh = x_hat[i];
    double d = (xh - (double)D[i]) / t_hat;
    if (dxg) d = d - (double)((wgt * dxg[i]) / gdiv);
    const double v = xh + (dt * d) * (mask ? (double)mask[i] : 1.0);
    d_cur[i] = d;
    x_next[i] = v;
    x32[i] = (float)v;
  }
}

// d' = (x_next - D')/t_next ; x_next = x_hat + (dt*(0.5 d + 0.5 d'))*mask   (mcedm.py:627-628)
__global__ void heun_correct_kernel(const double* __restrict__ x_hat, const double* __restrict__ d_cur,
                                    const float* __restrict__ D, const float* __restrict__ mask, double t_next, double dt,
                                    size_t total, double* __restrict__ x_next, float* __restrict__ x32,
                                    const float* __restrict__ dxg, float wgt, float gdiv) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    double dp = (x_next[i] - (double)D[i]) / t_next;
    if (dxg) dp = dp - (double)((wgt * dxg[i]) / gdiv);                 // models/ddim.py:1590-1591 (divides by t_hat here too)
    const double v = x_hat[i] + (dt * (0.5 * d_cur[i] + 0.5 * dp)) * (mask ? (double)mask[i] : 1.0);
    x_next[i] = v;
    x32[i] = (float)v;
  }
}

// 'b c h w -> b t h w c' for one time slot (mcedm.py:636-638)
__global__ void heun_store_kernel(const double* __restrict__ x, int C, size_t hw, int t, int T, size_t total,
                                  double* __restrict__ out) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    // i enumerates the OUTPUT (b, p, c) so stores are contiguous
    const size_t c = i % C;
    const size_t p = (i / C) % hw;
    const size_t b = i / (C * hw);
    out[((b * T + t) * hw + p) * C + c] = x[(b * C + c) * hw + p];
  }
}

int launch_heun_init(const float* cond, int cond_ch, int in_ch, size_t hw, const float* mask, const float* noise,
                     double t0, size_t total, double* x, float* x32, hipStream_t s) {
  hipLaunchKernelGGL(heun_init_kernel, dim3(grid_for(total)), dim3(256), 0, s, cond, cond_ch, in_ch, hw, mask, noise, t0,
                     total, x, x32);
  MCEDM_LAUNCH_CHECK("heun_init_kernel");
  return MCEDM_OK;
}
int launch_heun_churn(double* x, const double* eps, const float* mask, double c, size_t total, float* x32, hipStream_t s) {
  hipLaunchKernelGGL(heun_churn_kernel, dim3(grid_for(total)), dim3(256), 0, s, x, eps, mask, c, total, x32);
  MCEDM_LAUNCH_CHECK("heun_churn_kernel");
  return MCEDM_OK;
}
int launch_heun_euler(const double* x_hat, const float* D, const float* mask, double t_hat, double dt, size_t total,
                      double* d_cur, double* x_next, float* x32, hipStream_t s, const float* dxg, float wgt, float gdiv) {
  hipLaunchKernelGGL(heun_euler_kernel, dim3(grid_for(total)), dim3(256), 0, s, x_hat, D, mask, t_hat, dt, total, d_cur,
                     x_next, x32, dxg, wgt, gdiv);
  MCEDM_LAUNCH_CHECK("heun_euler_kernel");
  return MCEDM_OK;
}
int launch_heun_correct(const double* x_hat, const double* d_cur, const float* D, const float* mask, double t_next,
                        double dt, size_t total, double* x_next, float* x32, hipStream_t s, const float* dxg, float wgt,
                        float gdiv) {
  hipLaunchKernelGGL(heun_correct_kernel, dim3(grid_for(total)), dim3(256), 0, s, x_hat, d_cur, D, mask, t_next, dt,
                     total, x_next, x32, dxg, wgt, gdiv);
  MCEDM_LAUNCH_CHECK("heun_correct_kernel");
  return MCEDM_OK;
}
int launch_heun_store(const double* x, int C, size_t hw, int t, int T, size_t total, double* out, hipStream_t s) {
  hipLaunchKernelGGL(heun_store_kernel, dim3(grid_for(total)), dim3(256), 0, s, x, C, hw, t, T, total, out);
  MCEDM_LAUNCH_CHECK("heun_store_kernel");
  return MCEDM_OK;
}

// ---- counter-based normal noise on the device (Philox4x32-10, Salmon et al. 2011) -----------------------------------
// The reference draws one randn_like tensor per Heun step and per resampling loop (models/ddim.py:1004, 1037); at
// BASELINE config 5 (18 steps x 32 loops) that is 576 fp64 tensors per call.  Instead of materialising them, the
// re-noising kernel generates its own: counter = (element pair index, draw index), key = a 64-bit seed read from DEVICE
// memory (so a captured HIP graph replays with fresh noise after the host bumps the seed).  Statistically equivalent to,
// but not the same stream as, torch's generator.
__device__ __forceinline__ void philox4x32_10(unsigned (&c)[4], unsigned k0, unsigned k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned long long p0 = 0xD2511F53ull * c[0], p1 = 0xCD9E8D57ull * c[2];
    const unsigned n0 = (unsigned)(p1 >> 32) ^ c[1] ^ k0, n1 = (unsigned)p1;
    const unsigned n2 = (unsigned)(p0 >> 32) ^ c[3] ^ k1, n3 = (unsigned)p0;
    c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
}
// two independent N(0, 1) doubles from 128 random bits (Box-Muller on 53-bit uniforms; u1 in (0, 1])
__device__ __forceinline__ void normal_pair(const unsigned (&c)[4], double& z0, double& z1) {
  const double u1 = ((double)((((unsigned long long)c[0] << 32) | c[1]) >> 11) + 1.0) * (1.0 / 9007199254740992.0);
  const double u2 = (double)((((unsigned long long)c[2] << 32) | c[3]) >> 11) * (1.0 / 9007199254740992.0);
  const double r = sqrt(-2.0 * log(u1));
  double sn, cs;
  sincos(6.283185307179586476925 * u2, &sn, &cs);
  z0 = r * cs; z1 = r * sn;
}
// mask (optional): x_hat = x_cur + (c * eps) * mask, the joint model's churn (models/mcedm.py:608); NULL multiplies by 1.0 exactly
__global__ void heun_churn_rng_kernel(double* __restrict__ x, const unsigned long long* __restrict__ seed_dev,
                                      unsigned long long draw, double c, size_t total, float* __restrict__ x32,
                                      const float* __restrict__ mask) {
  const unsigned long long seed = *seed_dev;
  const size_t pairs = (total + 1) / 2;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < pairs; i += (size_t)gridDim.x * blockDim.x) {
    unsigned ctr[4] = {(unsigned)i, (unsigned)((unsigned long long)i >> 32), (unsigned)draw, (unsigned)(draw >> 32)};
    philox4x32_10(ctr, (unsigned)seed, (unsigned)(seed >> 32));
    double z0, z1;
    normal_pair(ctr, z0, z1);
    const double m0 = mask ? (double)mask[2 * i] : 1.0;
    const double v0 = x[2 * i] + (c * z0) * m0;
    x[2 * i] = v0; x32[2 * i] = (float)v0;
    if (2 * i + 1 < total) {
      const double m1 = mask ? (double)mask[2 * i + 1] : 1.0;
      const double v1 = x[2 * i + 1] + (c * z1) * m1;
      x[2 * i + 1] = v1; x32[2 * i + 1] = (float)v1;
    }
  }
}
int launch_heun_churn_rng(double* x, const unsigned long long* seed_dev, unsigned long long draw, double c, size_t total, float* x32,
                          hipStream_t s, const float* mask) {
  hipLaunchKernelGGL(heun_churn_rng_kernel, dim3(grid_for((total + 1) / 2)), dim3(256), 0, s, x, seed_dev, draw, c, total, x32, mask);
  MCEDM_LAUNCH_CHECK("heun_churn_rng_kernel");
  return MCEDM_OK;
}
// out[i] = N(0, 1) of draw `draw` (the generator on its own: tests, and callers that want the tensor)
__global__ void normal_fill_kernel(double* __restrict__ out, const unsigned long long* __restrict__ seed_dev, unsigned long long draw,
                                   size_t total) {
  const unsigned long long seed = *seed_dev;
  const size_t pairs = (total + 1) / 2;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < pairs; i += (size_t)gridDim.x * blockDim.x) {
    unsigned ctr[4] = {(unsigned)i, (unsigned)((unsigned long long)i >> 32), (unsigned)draw, (unsigned)(draw >> 32)};
    philox4x32_10(ctr, (unsigned)seed, (unsigned)(seed >> 32));
    double z0, z1;
    normal_pair(ctr, z0, z1);
    out[2 * i] = z0;
    if (2 * i + 1 < total) out[2 * i + 1] = z1;
  }
}
int launch_normal_fill(double* out, const unsigned long long* seed_dev, unsigned long long draw, size_t total, hipStream_t s) {
  hipLaunchKernelGGL(normal_fill_kernel, dim3(grid_for((total + 1) / 2)), dim3(256), 0, s, out, seed_dev, draw, total);
  MCEDM_LAUNCH_CHECK("normal_fill_kernel");
  return MCEDM_OK;
}

// ---- counter-based uniform noise (the DDIM samplers' torch.rand_like, models/ddim.py:893, 1512) ---------------------------
// Element e of draw d is word e % 4 of the Philox4x32-10 block with counter (lo32(e / 4), hi32(e / 4), lo32(d), hi32(d) | 2^31),
// key = the seed: the set top bit keeps these blocks apart from every block of the normal generator above, whose draw indices
// stay below 2^63.  u = (word >> 8) * 2^-24: fp32, in [0, 1), exact, torch.rand's granularity.  One block serves a 16-byte group.
__device__ __forceinline__ float4 uniform_group(unsigned long long seed, unsigned long long draw, size_t g) {
  unsigned ctr[4] = {(unsigned)g, (unsigned)((unsigned long long)g >> 32), (unsigned)draw, (unsigned)(draw >> 32) | 0x80000000u};
  philox4x32_10(ctr, (unsigned)seed, (unsigned)(seed >> 32));
  constexpr float k = 1.0f / 16777216.0f;
  return make_float4((float)(ctr[0] >> 8) * k, (float)(ctr[1] >> 8) * k, (float)(ctr[2] >> 8) * k, (float)(ctr[3] >> 8) * k);
}
// the same value for one element, whichever path asks for it (scalar tails, unaligned tensors)
__device__ __forceinline__ float uniform_element(unsigned long long seed, unsigned long long draw, size_t e) {
  const float4 u = uniform_group(seed, draw, e >> 2);
  const unsigned k = (unsigned)e & 3u;
  return k == 0 ? u.x : k == 1 ? u.y : k == 2 ? u.z : u.w;
}
// out[i] = U[0, 1) of draw `draw` (the generator on its own): n4 full groups stored as float4 (out 16-byte aligned), the rest
// element by element
__global__ void uniform_fill_kernel(float* __restrict__ out, const unsigned long long* __restrict__ seed_dev, unsigned long long draw,
                                    size_t n4, size_t total) {
  const unsigned long long seed = *seed_dev;
  const size_t tid = blockIdx.x * (size_t)blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
  for (size_t g = tid; g < n4; g += stride) reinterpret_cast<float4*>(out)[g] = uniform_group(seed, draw, g);
  for (size_t i = 4 * n4 + tid; i < total; i += stride) out[i] = uniform_element(seed, draw, i);
}
int launch_uniform_fill(float* out, const unsigned long long* seed_dev, unsigned long long draw, size_t total, hipStream_t s) {
  const size_t n4 = (reinterpret_cast<size_t>(out) & 15) == 0 ? total / 4 : 0;
  hipLaunchKernelGGL(uniform_fill_kernel, dim3(grid_for(n4 ? n4 : total)), dim3(256), 0, s, out, seed_dev, draw, n4, total);
  MCEDM_LAUNCH_CHECK("uniform_fill_kernel");
  return MCEDM_OK;
}

// ---- training-step dropout of the ADM U-Net (models/adm_blocks.py:170; the contract: mcedm_unet_plan_set_dropout) -------------
// keep iff u >= p; kept values times s = 1 / (1 - p), dropped values exactly zero.  Both kernels generate u themselves: one Philox
// block per 16-byte group, uniform_element for whatever a scalar path touches -- the value of an element never depends on the path.
__device__ __forceinline__ float drop_keep(float v, float u, float p, float s) { return u >= p ? v * s : 0.0f; }
__device__ __forceinline__ float drop_silu(float v, const Coef& c) {      // apply_coef's operations (conv_tile.hpp), SiLU on
  const float t = (v - c.mean) * c.scale + c.offset;
  return t * __builtin_amdgcn_rcpf(1.0f + __expf(-t));
}
// out = mask * s * silu(coef(h)): conv1's input of a dropout block.  grid = (planes, chunks of a plane) as act_materialize_kernel:
// one transform row per workgroup and 32-bit index arithmetic; plane (n, c) starts at element (n C + c) HW of the mask.  vec: HW % 4
// == 0 and 16-byte aligned tensors -- every group of four lies inside one plane; otherwise (15-pixel planes) element by element.
__global__ __launch_bounds__(256) void dropout_act_kernel(const float* __restrict__ h, const Coef* __restrict__ coef, int coef_batch,
                                                          int C, unsigned HW, float p, float s,
                                                          const unsigned long long* __restrict__ seed_dev, unsigned long long draw,
                                                          float* __restrict__ out, int vec) {
  const unsigned long long seed = *seed_dev;
  const int n = blockIdx.x / C, c = blockIdx.x - n * C;
  Coef cf{0.f, 1.f, 0.f, 0.f};
  if (coef) cf = coef[(coef_batch ? (size_t)n * C : 0) + c];
  const size_t e0 = (size_t)blockIdx.x * HW;
  const float* src = h + e0;
  float* dst = out + e0;
  if (vec) {
    const unsigned nq = HW / 4;
    const size_t g0 = e0 / 4;
    for (unsigned q = blockIdx.y * 256u + threadIdx.x; q < nq; q += gridDim.y * 256u) {
      const float4 v = reinterpret_cast<const float4*>(src)[q], u = uniform_group(seed, draw, g0 + q);
      float4 r;
      r.x = drop_keep(drop_silu(v.x, cf), u.x, p, s);
      r.y = drop_keep(drop_silu(v.y, cf), u.y, p, s);
      r.z = drop_keep(drop_silu(v.z, cf), u.z, p, s);
      r.w = drop_keep(drop_silu(v.w, cf), u.w, p, s);
      reinterpret_cast<float4*>(dst)[q] = r;
    }
  } else {
    for (unsigned i = blockIdx.y * 256u + threadIdx.x; i < HW; i += gridDim.y * 256u)
      dst[i] = drop_keep(drop_silu(src[i], cf), uniform_element(seed, draw, e0 + i), p, s);
  }
}
static int dropout_check_p(const char* who, double p) {
  MCEDM_REQUIRE(p > 0.0 && (float)p < 1.0f, "%s: p=%g must lie in (0, 1)", who, p);
  return MCEDM_OK;
}
int launch_dropout_act(const float* h, const Coef* coef, int coef_batch, float* out, int B, int C, int H, int W, double p,
                       const unsigned long long* seed_dev, unsigned long long draw, hipStream_t s) {
  MCEDM_REQUIRE(h && out && seed_dev && B > 0 && C > 0 && H > 0 && W > 0, "dropout_act: bad arguments");
  if (const int rc = dropout_check_p("dropout_act", p)) return rc;
  MCEDM_REQUIRE((size_t)B * C < (1ull << 31) && (size_t)H * W < (1ull << 31), "dropout_act: shape out of range");
  const unsigned HW = (unsigned)H * (unsigned)W;
  const int vec = HW % 4 == 0 && ((reinterpret_cast<size_t>(h) | reinterpret_cast<size_t>(out)) & 15) == 0;
  const unsigned per = vec ? HW / 4 : HW;
  int by = (int)((per + 1023) / 1024);                        // four trips per thread
  if (by < 1) by = 1;
  if (by > 64) by = 64;
  const float pf = (float)p;
  const double total = (double)B * C * HW;
  ProfScope ps("dropout_act_kernel", 14.0 * total, 8.0 * total, s);
  hipLaunchKernelGGL(dropout_act_kernel, dim3((unsigned)(B * C), (unsigned)by), dim3(256), 0, s, h, coef, coef_batch, C, HW, pf,
                     1.0f / (1.0f - pf), seed_dev, draw, out, vec);
  MCEDM_LAUNCH_CHECK("dropout_act_kernel");
  return MCEDM_OK;
}
// g = mask * s * g in place (the data gradient of conv1 on its way to the GroupNorm backward): n4 full groups as float4 (g 16-byte
// aligned), the rest element by element
__global__ __launch_bounds__(256) void dropout_scale_kernel(float* __restrict__ g, float p, float s,
                                                            const unsigned long long* __restrict__ seed_dev, unsigned long long draw,
                                                            size_t n4, size_t total) {
  const unsigned long long seed = *seed_dev;
  const size_t tid = blockIdx.x * (size_t)blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
  for (size_t q = tid; q < n4; q += stride) {
    const float4 v = reinterpret_cast<const float4*>(g)[q], u = uniform_group(seed, draw, q);
    reinterpret_cast<float4*>(g)[q] = make_float4(drop_keep(v.x, u.x, p, s), drop_keep(v.y, u.y, p, s), drop_keep(v.z, u.z, p, s),
                                                  drop_keep(v.w, u.w, p, s));
  }
  for (size_t i = 4 * n4 + tid; i < total; i += stride) g[i] = drop_keep(g[i], uniform_element(seed, draw, i), p, s);
}
int launch_dropout_scale(float* g, size_t total, double p, const unsigned long long* seed_dev, unsigned long long draw, hipStream_t s) {
  MCEDM_REQUIRE(g && seed_dev && total > 0, "dropout_scale: bad arguments");
  if (const int rc = dropout_check_p("dropout_scale", p)) return rc;
  const size_t n4 = (reinterpret_cast<size_t>(g) & 15) == 0 ? total / 4 : 0;
  const float pf = (float)p;
  ProfScope ps("dropout_scale_kernel", 12.0 * (double)total, 8.0 * (double)total, s);
  hipLaunchKernelGGL(dropout_scale_kernel, dim3(grid_for(n4 ? n4 : total)), dim3(256), 0, s, g, pf, 1.0f / (1.0f - pf), seed_dev, draw,
                     n4, total);
  MCEDM_LAUNCH_CHECK("dropout_scale_kernel");
  return MCEDM_OK;
}

// ---- RePaint-style EDM sampling on the DDPM U-Net (PlDdim, models/ddim.py:915-1051) -------------------------------
__global__ void vp_finish_kernel(const float* __restrict__ x, const float* __restrict__ F, float c_out, size_t total,
                                 float* __restrict__ D) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x)
    D[i] = 1.0f * x[i] + c_out * F[i];                                // c_skip * xt + c_out * F_x, ddim.py:945
}
int launch_vp_finish(const float* x, const float* F, float sigma, size_t total, float* D, hipStream_t s) {
  hipLaunchKernelGGL(vp_finish_kernel, dim3(grid_for(total)), dim3(256), 0, s, x, F, -sigma, total, D);
  MCEDM_LAUNCH_CHECK("vp_finish_kernel");
  return MCEDM_OK;
}

__global__ void vp_coef_kernel(float c_in, int n_self, int n_in, Coef* __restrict__ out) {
  const int c = threadIdx.x;
  if (c < n_self + n_in) out[c] = Coef{0.f, c < n_self ? 1.0f : c_in, 0.f, 0.f};
}
int launch_vp_coef(float c_in, int n_self, int n_in, Coef* out, hipStream_t s) {
  MCEDM_REQUIRE(n_self + n_in <= 64, "vp_coef: too many input channels");
  hipLaunchKernelGGL(vp_coef_kernel, dim3(1), dim3(64), 0, s, c_in, n_self, n_in, out);
  MCEDM_LAUNCH_CHECK("vp_coef_kernel");
  return MCEDM_OK;
}

// VP sampler of the ADM U-Net (PlCondDdim.sample_edm, models/ddim.py:1532-1601): one row set of conv_in transforms for
// cat(cond', x), every channel scaled by c_in (get_denoised scales x, cond and x_self_cond, :921-935), and the network's
// noise label c_noise written where the forward reads it
__global__ void vp_prepare_kernel(float c_in, int n_rows, int n_plain, float c_noise, Coef* __restrict__ coef,
                                  float* __restrict__ label) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c < n_rows + n_plain) coef[c] = Coef{0.f, c < n_rows ? c_in : 1.0f, 0.f, 0.f};
  if (c == 0) *label = c_noise;
}
int launch_vp_prepare(float c_in, int n_rows, float c_noise, Coef* coef, float* label, hipStream_t s, int n_plain) {
  hipLaunchKernelGGL(vp_prepare_kernel, dim3(ceil_div(n_rows + n_plain, 64)), dim3(64), 0, s, c_in, n_rows, n_plain, c_noise, coef,
                     label);
  MCEDM_LAUNCH_CHECK("vp_prepare_kernel");
  return MCEDM_OK;
}
// D = 1 * x + c_out * F, F = (w + 1) * F - w * F_uncond when Fu != NULL   (models/ddim.py:940-945)
__global__ void vp_cfg_finish_kernel(const float* __restrict__ x, const float* __restrict__ F, const float* __restrict__ Fu,
                                     float w1, float w, float c_out, size_t total, float* __restrict__ D) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    float f = F[i];
    if (Fu) f = w1 * f - w * Fu[i];
    D[i] = 1.0f * x[i] + c_out * f;
  }
}
int launch_vp_cfg_finish(const float* x, const float* F, const float* Fu, double w, float sigma, size_t total, float* D,
                         hipStream_t s) {
  hipLaunchKernelGGL(vp_cfg_finish_kernel, dim3(grid_for(total)), dim3(256), 0, s, x, F, Fu, (float)(w + 1.0), (float)w, -sigma,
                     total, D);
  MCEDM_LAUNCH_CHECK("vp_cfg_finish_kernel");
  return MCEDM_OK;
}

// EDM preconditioning around the DDPM U-Net (PlCondEdm.get_denoised, models/ddim.py:1745-1763) at one noise level:
// F = (w + 1) * F - w * F_uncond when Fu != NULL, D = c_skip * x + c_out * F; the blended F also to F_out when given
__global__ void edm_cfg_finish_kernel(const float* __restrict__ x, const float* __restrict__ F, const float* __restrict__ Fu,
                                      float w1, float w, float c_skip, float c_out, size_t total, float* __restrict__ D,
                                      float* __restrict__ F_out) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    float f = F[i];
    if (Fu) f = w1 * f - w * Fu[i];
    if (F_out) F_out[i] = f;
    D[i] = c_skip * x[i] + c_out * f;
  }
}
int launch_edm_cfg_finish(const float* x, const float* F, const float* Fu, double w, float c_skip, float c_out, size_t total,
                          float* D, float* F_out, hipStream_t s) {
  hipLaunchKernelGGL(edm_cfg_finish_kernel, dim3(grid_for(total)), dim3(256), 0, s, x, F, Fu, (float)(w + 1.0), (float)w, c_skip,
                     c_out, total, D, F_out);
  MCEDM_LAUNCH_CHECK("edm_cfg_finish_kernel");
  return MCEDM_OK;
}

// The same preconditioning with one noise level per sample (model_precond, models/ddim.py:1654-1666), every coefficient from
// sigma [B] in device memory, fp32 with the reference's expressions: row set b of conv_in's transform table scales the state
// channels by c_in(sigma_b) and leaves what conv_in reads in front of them alone; c_noise[b] = ln(sigma_b) / 4.
__global__ void edm_prepare_t_kernel(const float* __restrict__ sigma, float sigma_data, int n_front, int n_in, int B,
                                     Coef* __restrict__ coef, float* __restrict__ c_noise) {
  const int rows = n_front + n_in;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * rows) return;
  const int b = i / rows, c = i - b * rows;
  const float sg = sigma[b];
  const float c_in = 1.0f / sqrtf(sigma_data * sigma_data + sg * sg);
  coef[i] = Coef{0.f, c < n_front ? 1.0f : c_in, 0.f, 0.f};
  if (c == 0) c_noise[b] = logf(sg) / 4.0f;
}
int launch_edm_prepare_t(const float* sigma, float sigma_data, int n_front, int n_in, int B, Coef* coef, float* c_noise, hipStream_t s) {
  const int total = B * (n_front + n_in);
  hipLaunchKernelGGL(edm_prepare_t_kernel, dim3(ceil_div(total, 256)), dim3(256), 0, s, sigma, sigma_data, n_front, n_in, B, coef, c_noise);
  MCEDM_LAUNCH_CHECK("edm_prepare_t_kernel");
  return MCEDM_OK;
}
// D = c_skip(sigma_b) x + c_out(sigma_b) F, `per` elements per sample; F_out (optional, not F itself) <- F
__global__ void edm_finish_t_kernel(const float* __restrict__ x, const float* __restrict__ F, const float* __restrict__ sigma,
                                    float sigma_data, size_t per, size_t total, float* __restrict__ D, float* __restrict__ F_out) {
  const float sd2 = sigma_data * sigma_data;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const float sg = sigma[i / per], s2 = sg * sg;
    const float c_skip = sd2 / (s2 + sd2);
    const float c_out = sg * sigma_data / sqrtf(s2 + sd2);
    const float f = F[i];
    if (F_out) F_out[i] = f;
    D[i] = c_skip * x[i] + c_out * f;
  }
}
int launch_edm_finish_t(const float* x, const float* F, const float* sigma, float sigma_data, size_t per, size_t total, float* D,
                        float* F_out, hipStream_t s) {
  hipLaunchKernelGGL(edm_finish_t_kernel, dim3(grid_for(total)), dim3(256), 0, s, x, F, sigma, sigma_data, per, total, D, F_out);
  MCEDM_LAUNCH_CHECK("edm_finish_t_kernel");
  return MCEDM_OK;
}

__global__ void repaint_init_kernel(const float* __restrict__ hu, const float* __restrict__ noise,
                                    const float* __restrict__ mask, float sa, float sb, double t0, size_t total,
                                    double* __restrict__ x, float* __restrict__ x32) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const float m = mask[i], nz = noise[i];
    const float known = hu[i] * sa + nz * sb;                          // hu * aT.sqrt() + hu_noise * (1 - aT).sqrt(), fp32
    const float v32 = known * m + nz * (1.0f - m);
    const double v = (double)v32 * t0;
    x[i] = v;
    x32[i] = (float)v;
  }
}
int launch_repaint_init(const float* hu, const float* noise, const float* mask, float sa, float sb, double t0, size_t total,
                        double* x, float* x32, hipStream_t s) {
  hipLaunchKernelGGL(repaint_init_kernel, dim3(grid_for(total)), dim3(256), 0, s, hu, noise, mask, sa, sb, t0, total, x, x32);
  MCEDM_LAUNCH_CHECK("repaint_init_kernel");
  return MCEDM_OK;
}

__global__ void repaint_known_kernel(double* __restrict__ x, const float* __restrict__ hu, const float* __restrict__ noise,
                                     const float* __restrict__ mask, float sa, float sb, int final_clean, size_t total,
                                     float* __restrict__ x32) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const float m = mask[i];
    // at_next.sqrt() * hu + (1 - at_next).sqrt() * hu_noise in fp32; the final replacement uses the clean hu
    const float known = final_clean ? hu[i] : sa * hu[i] + sb * noise[i];
    const float km = known * m;                                        // fp32 * fp32
    const double v = (double)km + x[i] * (double)(1.0f - m);           // fp64 * fp32 promotes to fp64
    x[i] = v;
    x32[i] = (float)v;
  }
}
int launch_repaint_known(double* x, const float* hu, const float* noise, const float* mask, float sa, float sb, int final_clean,
                         size_t total, float* x32, hipStream_t s) {
  hipLaunchKernelGGL(repaint_known_kernel, dim3(grid_for(total)), dim3(256), 0, s, x, hu, noise, mask, sa, sb, final_clean,
                     total, x32);
  MCEDM_LAUNCH_CHECK("repaint_known_kernel");
  return MCEDM_OK;
}

// ---- DDIM sampler with RePaint loops (PlDdim.sample_with_repeat, models/ddim.py:808-913): fp32 like the reference ----
__global__ void ddim_x0_kernel(float* __restrict__ xt, const float* __restrict__ et, const float* __restrict__ hu,
                               const float* __restrict__ mask, float s0, float s1, int renoise, size_t total,
                               float* __restrict__ x0) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const float e = et[i], m = mask[i];
    float v = (xt[i] - e * s1) / s0;                                   // (xt - et * (1 - at).sqrt()) / at.sqrt()
    v = hu[i] * m + v * (1.0f - m);                                    // add known part (:878-879)
    x0[i] = v;
    if (renoise) xt[i] = s0 * v + s1 * e;                              // at.sqrt() * x0_t + (1 - at).sqrt() * et (:881-882)
  }
}
int launch_ddim_x0(float* xt, const float* et, const float* hu, const float* mask, float s0, float s1, int renoise, size_t total,
                   float* x0, hipStream_t s) {
  hipLaunchKernelGGL(ddim_x0_kernel, dim3(grid_for(total)), dim3(256), 0, s, xt, et, hu, mask, s0, s1, renoise, total, x0);
  MCEDM_LAUNCH_CHECK("ddim_x0_kernel");
  return MCEDM_OK;
}
__global__ void ddim_next_kernel(const float* __restrict__ x0, const float* __restrict__ et, const float* __restrict__ hu,
                                 const float* __restrict__ hn, const float* __restrict__ mask, const float* __restrict__ noise,
                                 float sa, float c1, float c2, size_t total, float* __restrict__ xt) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const float m = mask[i];
    float v = noise ? (sa * x0[i] + c1 * noise[i]) + c2 * et[i] : sa * x0[i] + c2 * et[i];      // (:891-895)
    const float known = sa * hu[i] + c2 * hn[i];                                                // at_next.sqrt() * hu + c2 * hu_noise
    xt[i] = known * m + v * (1.0f - m);
  }
}
int launch_ddim_next(const float* x0, const float* et, const float* hu, const float* hn, const float* mask, const float* noise,
                     float sa, float c1, float c2, size_t total, float* xt, hipStream_t s) {
  hipLaunchKernelGGL(ddim_next_kernel, dim3(grid_for(total)), dim3(256), 0, s, x0, et, hu, hn, mask, noise, sa, c1, c2, total, xt);
  MCEDM_LAUNCH_CHECK("ddim_next_kernel");
  return MCEDM_OK;
}
// The same step with the uniform draw generated in the kernel (launch_ddim_next_rng): every thread takes four consecutive
// elements -- one Philox block, 16-byte loads and one 16-byte store -- for the n4 full groups (all pointers 16-byte aligned), the
// rest element by element with the value uniform_fill_kernel writes for that element.
__device__ __forceinline__ float ddim_next_point(float x0, float et, float hu, float hn, float m, float nz, float sa, float c1, float c2) {
  const float v = (sa * x0 + c1 * nz) + c2 * et;
  const float known = sa * hu + c2 * hn;
  return known * m + v * (1.0f - m);
}
__global__ __launch_bounds__(256) void ddim_next_rng_kernel(const float* __restrict__ x0, const float* __restrict__ et,
                                                            const float* __restrict__ hu, const float* __restrict__ hn,
                                                            const float* __restrict__ mask,
                                                            const unsigned long long* __restrict__ seed_dev, unsigned long long draw,
                                                            float sa, float c1, float c2, size_t n4, size_t total, float* __restrict__ xt) {
  const unsigned long long seed = *seed_dev;
  const size_t tid = blockIdx.x * (size_t)blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
  for (size_t g = tid; g < n4; g += stride) {
    const float4 a = reinterpret_cast<const float4*>(x0)[g], e = reinterpret_cast<const float4*>(et)[g];
    const float4 h = reinterpret_cast<const float4*>(hu)[g], n = reinterpret_cast<const float4*>(hn)[g];
    const float4 m = reinterpret_cast<const float4*>(mask)[g], u = uniform_group(seed, draw, g);
    float4 r;
    r.x = ddim_next_point(a.x, e.x, h.x, n.x, m.x, u.x, sa, c1, c2);
    r.y = ddim_next_point(a.y, e.y, h.y, n.y, m.y, u.y, sa, c1, c2);
    r.z = ddim_next_point(a.z, e.z, h.z, n.z, m.z, u.z, sa, c1, c2);
    r.w = ddim_next_point(a.w, e.w, h.w, n.w, m.w, u.w, sa, c1, c2);
    reinterpret_cast<float4*>(xt)[g] = r;
  }
  for (size_t i = 4 * n4 + tid; i < total; i += stride)
    xt[i] = ddim_next_point(x0[i], et[i], hu[i], hn[i], mask[i], uniform_element(seed, draw, i), sa, c1, c2);
}
int launch_ddim_next_rng(const float* x0, const float* et, const float* hu, const float* hn, const float* mask,
                         const unsigned long long* seed_dev, unsigned long long draw, float sa, float c1, float c2, size_t total,
                         float* xt, hipStream_t s) {
  auto al16 = [](const void* p) { return (reinterpret_cast<size_t>(p) & 15) == 0; };
  const size_t n4 = al16(x0) && al16(et) && al16(hu) && al16(hn) && al16(mask) && al16(xt) ? total / 4 : 0;
  hipLaunchKernelGGL(ddim_next_rng_kernel, dim3(grid_for(n4 ? n4 : total)), dim3(256), 0, s, x0, et, hu, hn, mask, seed_dev, draw, sa,
                     c1, c2, n4, total, xt);
  MCEDM_LAUNCH_CHECK("ddim_next_rng_kernel");
  return MCEDM_OK;
}
__global__ void ddim_init_kernel(const float* __restrict__ hu, const float* __restrict__ hn, const float* __restrict__ mask,
                                 float sa, float sb, size_t total, float* __restrict__ xt) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const float m = mask[i], nz = hn[i];
    xt[i] = (hu[i] * sa + nz * sb) * m + nz * (1.0f - m);             // ddim.py:837-838
  }
}
int launch_ddim_init(const float* hu, const float* hn, const float* mask, float sa, float sb, size_t total, float* xt, hipStream_t s) {
  hipLaunchKernelGGL(ddim_init_kernel, dim3(grid_for(total)), dim3(256), 0, s, hu, hn, mask, sa, sb, total, xt);
  MCEDM_LAUNCH_CHECK("ddim_init_kernel");
  return MCEDM_OK;
}
__global__ void store_f32_kernel(const float* __restrict__ x, int C, size_t hw, int t, int T, size_t total, float* __restrict__ out) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const size_t c = i % C, p = (i / C) % hw, b = i / (C * hw);
    out[((b * T + t) * hw + p) * C + c] = x[(b * C + c) * hw + p];
  }
}
int launch_store_f32(const float* x, int C, size_t hw, int t, int T, size_t total, float* out, hipStream_t s) {
  hipLaunchKernelGGL(store_f32_kernel, dim3(grid_for(total)), dim3(256), 0, s, x, C, hw, t, T, total, out);
  MCEDM_LAUNCH_CHECK("store_f32_kernel");
  return MCEDM_OK;
}

// ---- DDIM sampler of the conditional ADM U-Net (PlCondDdim.sample, models/ddim.py:1452-1530): one pass per step --------
// fp32 in the reference's order (:1497-1515; this file is built without fma contraction).  Pure streaming: every thread
// takes four consecutive state elements (16-byte loads of xt / F / Fu / noise, 16-byte store of xt_next) and scatters x0
// and xt_next to where their readers want them -- the self-conditioning channels of cond' and of its zero-cond twin
// ([B, Cp, H, W]: the next forward's conv_in reads them there) and one slot each of the 'b t h w c' trajectories.
// PDE guidance (dxg, C == 1): et = fl(et - fl(gw * dx)) in front of x0 (:1502-1503), dx at the state's own index.
__device__ __forceinline__ void ddim_cond_point(const DdimCondStep& a, float x, float f, float fu, float nz, float dx, float& x0, float& xn) {
  float et = a.Fu ? a.w1 * f - a.w * fu : f;                           // (w + 1) * model(cond) - w * model(None)   (:1497)
  if (a.dxg) et = et - a.gw * dx;                                      // et - 5. * (1 - at).sqrt() * dx            (:1502-1503)
  x0 = (x - et * a.s1) / a.s0;                                         // (xt - et * (1 - at).sqrt()) / at.sqrt()   (:1505)
  xn = (a.noise || a.seed) ? (a.sa * x0 + a.c1 * nz) + a.c2 * et : a.sa * x0 + a.c2 * et;        // (:1512 / :1515)
}
// element i of the [B, C, H, W] state -> its places in cond' / twin and in the trajectories
__device__ __forceinline__ void ddim_cond_scatter(const DdimCondStep& a, size_t i, float x0, float xn) {
  const size_t chw = (size_t)a.C * a.hw, b = i / chw, r = i - b * chw;
  if (a.sc) {
    const size_t j = (b * (size_t)a.Cp + (size_t)a.sc_off) * a.hw + r;
    a.sc[j] = x0;
    if (a.sc_u) a.sc_u[j] = x0;
  }
  if (a.xs || a.x0s) {
    const size_t c = r / a.hw, p = r - c * a.hw;
    if (a.xs) a.xs[((b * (size_t)a.T_xs + (size_t)a.t_xs) * a.hw + p) * (size_t)a.C + c] = xn;
    if (a.x0s) a.x0s[((b * (size_t)a.T_x0 + (size_t)a.t_x0) * a.hw + p) * (size_t)a.C + c] = x0;
  }
}
__global__ __launch_bounds__(256) void ddim_cond_step_kernel(DdimCondStep a, size_t n4, int vec_sc, int vec_tr) {
  const size_t tid = blockIdx.x * (size_t)blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
  const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
  const unsigned long long seed = a.seed ? *a.seed : 0ull;             // the draws come from the generator: no noise load
  for (size_t g = tid; g < n4; g += stride) {
    const float4 x = reinterpret_cast<const float4*>(a.xt)[g], f = reinterpret_cast<const float4*>(a.F)[g];
    const float4 fu = a.Fu ? reinterpret_cast<const float4*>(a.Fu)[g] : zero4;
    const float4 nz = a.seed ? uniform_group(seed, a.draw, g) : a.noise ? reinterpret_cast<const float4*>(a.noise)[g] : zero4;
    const float4 dx = a.dxg ? reinterpret_cast<const float4*>(a.dxg)[g] : zero4;      // C == 1: the state's own index
    float4 x0, xn;
    ddim_cond_point(a, x.x, f.x, fu.x, nz.x, dx.x, x0.x, xn.x);
    ddim_cond_point(a, x.y, f.y, fu.y, nz.y, dx.y, x0.y, xn.y);
    ddim_cond_point(a, x.z, f.z, fu.z, nz.z, dx.z, x0.z, xn.z);
    ddim_cond_point(a, x.w, f.w, fu.w, nz.w, dx.w, x0.w, xn.w);
    reinterpret_cast<float4*>(a.xt_next)[g] = xn;
    const size_t i = 4 * g;
    // H * W % 4 == 0: the four elements share (b, c) and every destination offset is a multiple of four
    const size_t chw = (size_t)a.C * a.hw, b = i / chw, r = i - b * chw;
    if (a.sc) {
      if (vec_sc) {
        const size_t j = (b * (size_t)a.Cp + (size_t)a.sc_off) * a.hw + r;
        *reinterpret_cast<float4*>(a.sc + j) = x0;
        if (a.sc_u) *reinterpret_cast<float4*>(a.sc_u + j) = x0;
      } else {
        DdimCondStep t = a; t.xs = nullptr; t.x0s = nullptr;
        ddim_cond_scatter(t, i, x0.x, xn.x); ddim_cond_scatter(t, i + 1, x0.y, xn.y);
        ddim_cond_scatter(t, i + 2, x0.z, xn.z); ddim_cond_scatter(t, i + 3, x0.w, xn.w);
      }
    }
    if (a.xs || a.x0s) {
      if (vec_tr) {                      // C == 1: a sample's slot is contiguous
        if (a.xs) *reinterpret_cast<float4*>(a.xs + (b * (size_t)a.T_xs + (size_t)a.t_xs) * a.hw + r) = xn;
        if (a.x0s) *reinterpret_cast<float4*>(a.x0s + (b * (size_t)a.T_x0 + (size_t)a.t_x0) * a.hw + r) = x0;
      } else {
        DdimCondStep t = a; t.sc = nullptr;
        ddim_cond_scatter(t, i, x0.x, xn.x); ddim_cond_scatter(t, i + 1, x0.y, xn.y);
        ddim_cond_scatter(t, i + 2, x0.z, xn.z); ddim_cond_scatter(t, i + 3, x0.w, xn.w);
      }
    }
  }
  for (size_t i = 4 * n4 + tid; i < a.n; i += stride) {                // scalar tail (everything, when a pointer is not 16-byte aligned)
    float x0, xn;
    const float nz = a.seed ? uniform_element(seed, a.draw, i) : a.noise ? a.noise[i] : 0.f;
    ddim_cond_point(a, a.xt[i], a.F[i], a.Fu ? a.Fu[i] : 0.f, nz, a.dxg ? a.dxg[i] : 0.f, x0, xn);
    a.xt_next[i] = xn;
    ddim_cond_scatter(a, i, x0, xn);
  }
}
int launch_ddim_cond_step(const DdimCondStep& a, hipStream_t s) {
  auto al16 = [](const void* p) { return (reinterpret_cast<size_t>(p) & 15) == 0; };
  const bool body = al16(a.xt) && al16(a.F) && al16(a.Fu) && al16(a.noise) && al16(a.dxg) && al16(a.xt_next);
  const size_t n4 = body ? a.n / 4 : 0;
  const int vec_sc = a.hw % 4 == 0 && al16(a.sc) && al16(a.sc_u);
  const int vec_tr = a.hw % 4 == 0 && a.C == 1 && al16(a.xs) && al16(a.x0s);
  hipLaunchKernelGGL(ddim_cond_step_kernel, dim3(grid_for(n4 ? n4 : a.n)), dim3(256), 0, s, a, n4, vec_sc, vec_tr);
  MCEDM_LAUNCH_CHECK("ddim_cond_step_kernel");
  return MCEDM_OK;
}

// ---- training-side elementwise ----------------------------------------------------------------
// sigma = exp(rnd*P_std + P_mean) (mcedm.py:271); x_noise = x + mask*noise*sigma (mcedm.py:216)
__global__ void noise_inputs_kernel(const float* __restrict__ x, const float* __restrict__ mask,
                                    const float* __restrict__ noise, const float* __restrict__ rnd, float P_mean,
                                    float P_std, size_t per_sample, size_t total, float* __restrict__ x_noise,
                                    float* __restrict__ sigma_out) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const size_t b = i / per_sample;
    const float sigma = expf(rnd[b] * P_std + P_mean);
    if (i % per_sample == 0) sigma_out[b] = sigma;
    x_noise[i] = mask ? x[i] + mask[i] * noise[i] * sigma : x[i] + noise[i] * sigma;      // mcedm.py:216-218
  }
}

// ---- epsilon-prediction training (PlCondDdim, models/ddim.py:195-226, 1118-1152) ------------------------------------
// x_noise = x * sqrt(a_t) + noise * sqrt(1 - a_t), labels = t.float()   (models/ddim.py:195-197, 209)
__global__ void eps_noise_inputs_kernel(const float* __restrict__ x, const float* __restrict__ noise,
                                        const int64_t* __restrict__ t, const float* __restrict__ sqrt_ab,
                                        const float* __restrict__ sqrt_1mab, int n_table, size_t per_sample, size_t total,
                                        float* __restrict__ x_noise, float* __restrict__ labels) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const size_t b = i / per_sample;
    int64_t tb = t[b];
    tb = tb < 0 ? 0 : (tb >= n_table ? n_table - 1 : tb);           // the host checks the range; never read out of the table
    if (i % per_sample == 0) labels[b] = (float)t[b];
    x_noise[i] = x[i] * sqrt_ab[tb] + noise[i] * sqrt_1mab[tb];
  }
}

// cond' = cat(cond or 0, x_sc or 0), x_sc = (x_noise - F0 * sqrt(1 - a_t)) / sqrt(a_t)   (models/ddim.py:205-210)
__global__ void eps_self_cond_kernel(const float* __restrict__ x_noise, const float* __restrict__ F0,
                                     const int64_t* __restrict__ t, const float* __restrict__ sqrt_ab,
                                     const float* __restrict__ sqrt_1mab, int n_table, const float* __restrict__ cond,
                                     int cond_ch, int in_ch, size_t hw, size_t total, float* __restrict__ out) {
  const int Ct = cond_ch + in_ch;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const size_t p = i % hw, c = (i / hw) % Ct, b = i / (hw * Ct);
    float v = 0.0f;
    if ((int)c < cond_ch) {
      if (cond) v = cond[(b * cond_ch + c) * hw + p];
    } else if (F0) {
      int64_t tb = t[b];
      tb = tb < 0 ? 0 : (tb >= n_table ? n_table - 1 : tb);
      const size_t j = (b * in_ch + (c - cond_ch)) * hw + p;
      v = (x_noise[j] - F0[j] * sqrt_1mab[tb]) / sqrt_ab[tb];
    }
    out[i] = v;
  }
}

// (the deterministic grid-wide sum these kernels end with, grid_sum_fixed_order, lives in edm.hpp: pde.hip uses it too)
// loss = mean_b sum_chw w_b*(D*m - x*m)^2 ; dD = (2 w_b / B) * (D*m - x*m) * m   (mcedm.py:278, losses.py:48-53)
__global__ __launch_bounds__(256) void edm_loss_kernel(const float* __restrict__ D, const float* __restrict__ x,
                                                       const float* __restrict__ mask, const float* __restrict__ sigma,
                                                       float sigma_data, int B, size_t per_sample,
                                                       float* __restrict__ loss, float* __restrict__ dD, RedScratch rs) {
  const int b = blockIdx.y;
  const float s = sigma[b];
  const float wgt = (s * s + sigma_data * sigma_data) / ((s * sigma_data) * (s * sigma_data));
  const size_t base = (size_t)b * per_sample;
  float acc = 0.f;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < per_sample; i += (size_t)gridDim.x * blockDim.x) {
    const float m = mask ? mask[base + i] : 1.0f;
    const float diff = D[base + i] * m - x[base + i] * m;
    acc += wgt * (diff * diff);
    if (dD) dD[base + i] = (2.0f * wgt / (float)B) * diff * m;
  }
  double t = acc;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) t += __shfl_xor(t, off);
  __shared__ double red[4];
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = t;
  __syncthreads();
  double total;
  if (grid_sum_fixed_order(rs, (red[0] + red[1]) + (red[2] + red[3]), blockIdx.y * gridDim.x + blockIdx.x, gridDim.x * gridDim.y, &total) &&
      threadIdx.x == 0)
    *loss = (float)(total / (double)B);
}

// NoiseEstimationLoss: loss = mean_b sum_chw (F - eps)^2 ; dF = (2 / B) (F - eps)   (models/losses.py:39-59)
__global__ __launch_bounds__(256) void eps_loss_kernel(const float* __restrict__ F, const float* __restrict__ eps, int B,
                                                       size_t per_sample, float* __restrict__ loss, float* __restrict__ dF,
                                                       RedScratch rs) {
  const int b = blockIdx.y;
  const size_t base = (size_t)b * per_sample;
  float acc = 0.f;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < per_sample; i += (size_t)gridDim.x * blockDim.x) {
    const float diff = F[base + i] - eps[base + i];
    acc += diff * diff;
    if (dF) dF[base + i] = (2.0f / (float)B) * diff;
  }
  double t = acc;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) t += __shfl_xor(t, off);
  __shared__ double red[4];
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = t;
  __syncthreads();
  double total;
  if (grid_sum_fixed_order(rs, (red[0] + red[1]) + (red[2] + red[3]), blockIdx.y * gridDim.x + blockIdx.x, gridDim.x * gridDim.y, &total) &&
      threadIdx.x == 0)
    *loss = (float)(total / (double)B);
}

__global__ __launch_bounds__(256) void sqnorm_kernel(const float* __restrict__ g, size_t n, double* __restrict__ out, RedScratch rs) {
  float a0 = 0.f, a1 = 0.f;
  size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (; i + stride < n; i += 2 * stride) {
    const float u = g[i], v = g[i + stride];
    a0 += u * u; a1 += v * v;
  }
  if (i < n) { const float u = g[i]; a0 += u * u; }
  double t = (double)a0 + (double)a1;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) t += __shfl_xor(t, off);
  __shared__ double red[4];
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = t;
  __syncthreads();
  double total;
  if (grid_sum_fixed_order(rs, (red[0] + red[1]) + (red[2] + red[3]), blockIdx.x, gridDim.x, &total) && threadIdx.x == 0) *out = total;
}

// torch.optim.Adam (no amsgrad) on clipped grads, then EmaModel.update (ddim_blocks.py:44-54).
__global__ void adam_ema_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                float* __restrict__ v, float* __restrict__ ema, size_t n, float step_size, float w1,
                                float b2, float w2, float eps, float wd, const double* __restrict__ sqnorm,
                                double max_norm, float gscale, float ema_beta, float ema_w, float bc2_sqrt) {
  float clip = 1.f;
  if (sqnorm) {
    // clip_grad_norm_: coef = max_norm / (total_norm + 1e-6), clamped to 1; norm of the (scaled) grads
    const double total = sqrt(*sqnorm) * (double)gscale;
    const double c = max_norm / (total + 1e-6);
    clip = (float)(c < 1.0 ? c : 1.0);
  }
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    float gi = g[i] * gscale * clip;
    const float pi = p[i];
    if (wd != 0.f) gi += wd * pi;
    // exp_avg.lerp_(grad, 1-b1); exp_avg_sq.mul_(b2).addcmul_(grad, grad, value=1-b2); addcdiv_(m, denom, -step_size)
    const float m0 = m[i];
    const float mi = m0 + w1 * (gi - m0);
    const float vi = v[i] * b2 + w2 * (gi * gi);
    const float denom = sqrtf(vi) / bc2_sqrt + eps;
    const float pn = pi - step_size * (mi / denom);
    m[i] = mi; v[i] = vi; p[i] = pn;
    if (ema) ema[i] = ema[i] * ema_beta + ema_w * pn;
  }
}

}  // namespace mcedm

using namespace mcedm;

extern "C" int mcedm_edm_noise_inputs(const float* x, const float* mask, const float* noise, const float* rnd_normal,
                                      int B, int C, int H, int W, double P_mean, double P_std, float* x_noise,
                                      float* sigma_out, void* stream) {
  MCEDM_REQUIRE(x && noise && rnd_normal && x_noise && sigma_out, "noise_inputs: null pointer");
  MCEDM_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0, "noise_inputs: empty shape");
  const size_t per = (size_t)C * H * W, total = per * B;
  hipLaunchKernelGGL(noise_inputs_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, x, mask, noise,
                     rnd_normal, (float)P_mean, (float)P_std, per, total, x_noise, sigma_out);
  MCEDM_LAUNCH_CHECK("noise_inputs_kernel");
  return MCEDM_OK;
}

extern "C" int mcedm_edm_loss(const float* D, const float* x, const float* mask, const float* sigma, int B, int C, int H,
                              int W, double sigma_data, float* loss_out, float* dD_out, void* scratch, size_t scratch_bytes,
                              void* stream) {
  MCEDM_REQUIRE(D && x && sigma && loss_out, "edm_loss: null pointer");
  MCEDM_REQUIRE(scratch && scratch_bytes >= MCEDM_REDUCE_SCRATCH_BYTES && ((size_t)scratch & 7) == 0,
                "edm_loss: needs %d bytes of 8-byte aligned device scratch (MCEDM_REDUCE_SCRATCH_BYTES)", MCEDM_REDUCE_SCRATCH_BYTES);
  MCEDM_REQUIRE(B > 0 && B <= 65535 && C > 0 && H > 0 && W > 0, "edm_loss: bad shape");
  const size_t per = (size_t)C * H * W;
  MCEDM_REQUIRE(B <= RED_MAX, "edm_loss: batch %d exceeds the reduction table (%d)", B, RED_MAX);
  int gx = (int)((per + 255) / 256);
  if (gx > 64) gx = 64;
  if (gx > RED_MAX / B) gx = RED_MAX / B;            // one slot of the fixed-order reduction per block
  const RedScratch rs = red_scratch(scratch);
  MCEDM_HIP_TRY(hipMemsetAsync(rs.ticket, 0, sizeof(unsigned), (hipStream_t)stream));
  hipLaunchKernelGGL(edm_loss_kernel, dim3(gx, B), dim3(256), 0, (hipStream_t)stream, D, x, mask, sigma,
                     (float)sigma_data, B, per, loss_out, dD_out, rs);
  MCEDM_LAUNCH_CHECK("edm_loss_kernel");
  return MCEDM_OK;
}

extern "C" int mcedm_eps_noise_inputs(const float* x, const float* noise, const int64_t* t, const float* sqrt_ab,
                                      const float* sqrt_1mab, int n_table, int B, int C, int H, int W, float* x_noise,
                                      float* labels, void* stream) {
  MCEDM_REQUIRE(x && noise && t && sqrt_ab && sqrt_1mab && x_noise && labels, "eps_noise_inputs: null pointer");
  MCEDM_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0 && n_table > 0, "eps_noise_inputs: empty shape");
  const size_t per = (size_t)C * H * W, total = per * B;
  hipLaunchKernelGGL(eps_noise_inputs_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, x, noise, t, sqrt_ab,
                     sqrt_1mab, n_table, per, total, x_noise, labels);
  MCEDM_LAUNCH_CHECK("eps_noise_inputs_kernel");
  return MCEDM_OK;
}

extern "C" int mcedm_eps_self_cond(const float* x_noise, const float* F0, const int64_t* t, const float* sqrt_ab,
                                   const float* sqrt_1mab, int n_table, const float* cond, int cond_channels, int in_channels,
                                   int B, int H, int W, float* cond_out, void* stream) {
  MCEDM_REQUIRE(cond_out, "eps_self_cond: null output");
  MCEDM_REQUIRE(!F0 || (x_noise && t && sqrt_ab && sqrt_1mab && n_table > 0), "eps_self_cond: F0 needs x_noise, t and the tables");
  MCEDM_REQUIRE(B > 0 && H > 0 && W > 0 && cond_channels >= 0 && in_channels >= 0 && cond_channels + in_channels > 0, "eps_self_cond: bad shape");
  const size_t hw = (size_t)H * W, total = (size_t)B * (cond_channels + in_channels) * hw;
  hipLaunchKernelGGL(eps_self_cond_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, x_noise, F0, t, sqrt_ab,
                     sqrt_1mab, n_table, cond, cond_channels, in_channels, hw, total, cond_out);
  MCEDM_LAUNCH_CHECK("eps_self_cond_kernel");
  return MCEDM_OK;
}

extern "C" int mcedm_eps_loss(const float* F, const float* eps, int B, int C, int H, int W, float* loss_out, float* dF_out,
                              void* scratch, size_t scratch_bytes, void* stream) {
  MCEDM_REQUIRE(F && eps && loss_out, "eps_loss: null pointer");
  MCEDM_REQUIRE(scratch && scratch_bytes >= MCEDM_REDUCE_SCRATCH_BYTES && ((size_t)scratch & 7) == 0,
                "eps_loss: needs %d bytes of 8-byte aligned device scratch (MCEDM_REDUCE_SCRATCH_BYTES)", MCEDM_REDUCE_SCRATCH_BYTES);
  MCEDM_REQUIRE(B > 0 && B <= 65535 && C > 0 && H > 0 && W > 0, "eps_loss: bad shape");
  MCEDM_REQUIRE(B <= RED_MAX, "eps_loss: batch %d exceeds the reduction table (%d)", B, RED_MAX);
  const size_t per = (size_t)C * H * W;
  int gx = (int)((per + 255) / 256);                 // the same grid as mcedm_edm_loss
  if (gx > 64) gx = 64;
  if (gx > RED_MAX / B) gx = RED_MAX / B;
  const RedScratch rs = red_scratch(scratch);
  MCEDM_HIP_TRY(hipMemsetAsync(rs.ticket, 0, sizeof(unsigned), (hipStream_t)stream));
  hipLaunchKernelGGL(eps_loss_kernel, dim3(gx, B), dim3(256), 0, (hipStream_t)stream, F, eps, B, per, loss_out, dF_out, rs);
  MCEDM_LAUNCH_CHECK("eps_loss_kernel");
  return MCEDM_OK;
}

extern "C" int mcedm_sqnorm(const float* g, size_t n, double* sqnorm_out, void* scratch, size_t scratch_bytes, void* stream) {
  MCEDM_REQUIRE(g && sqnorm_out, "sqnorm: null pointer");
  MCEDM_REQUIRE(scratch && scratch_bytes >= MCEDM_REDUCE_SCRATCH_BYTES && ((size_t)scratch & 7) == 0,
                "sqnorm: needs %d bytes of 8-byte aligned device scratch (MCEDM_REDUCE_SCRATCH_BYTES)", MCEDM_REDUCE_SCRATCH_BYTES);
  if (n == 0) { MCEDM_HIP_TRY(hipMemsetAsync(sqnorm_out, 0, sizeof(double), (hipStream_t)stream)); return MCEDM_OK; }
  int blocks = grid_for(n);
  if (blocks > RED_MAX) blocks = RED_MAX;
  const RedScratch rs = red_scratch(scratch);
  MCEDM_HIP_TRY(hipMemsetAsync(rs.ticket, 0, sizeof(unsigned), (hipStream_t)stream));
  hipLaunchKernelGGL(sqnorm_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, g, n, sqnorm_out, rs);
  MCEDM_LAUNCH_CHECK("sqnorm_kernel");
  return MCEDM_OK;
}

extern "C" int mcedm_adam_ema_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float* ema,
                                   size_t n, double lr, double beta1, double beta2, double eps, double weight_decay,
                                   const double* sqnorm, double max_norm, double grad_scale, double ema_beta,
                                   int64_t step, void* stream) {
  MCEDM_REQUIRE(param && grad && exp_avg && exp_avg_sq, "adam: null pointer");
  MCEDM_REQUIRE(step >= 1, "adam: step counts from 1 (got %lld)", (long long)step);
  if (n == 0) return MCEDM_OK;
  const double bc1 = 1.0 - pow(beta1, (double)step);
  const double bc2 = 1.0 - pow(beta2, (double)step);
  // scalar factors are formed in double on the host exactly as torch.optim.Adam / EmaModel form them in Python
  hipLaunchKernelGGL(adam_ema_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, param, grad, exp_avg,
                     exp_avg_sq, ema, n, (float)(lr / bc1), (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2),
                     (float)eps, (float)weight_decay, sqnorm, max_norm, (float)grad_scale, (float)ema_beta,
                     (float)(1.0 - ema_beta), (float)sqrt(bc2));
  MCEDM_LAUNCH_CHECK("adam_ema_kernel");
  return MCEDM_OK;
}
