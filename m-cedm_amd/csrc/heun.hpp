// heun.hpp -- what the three Heun samplers share (EDM and VP on the ADM U-Net: sampler.hip; RePaint on the DDPM U-Net:
// ddpm.hip): the five state buffers in front of the network's workspace, the trajectory stores, the churn and the
// 2nd-order update.  Each sampler keeps its own schedule arithmetic (fp64, on the host), decides itself whether a step
// churns, and passes its network in as a callable.
#pragma once
#include <utility>

#include "edm.hpp"
#include "plan.hpp"

namespace mcedm {

// byte offsets of the fp64 state x, the next state xn, the Euler slope d, and of the fp32 network input x32 and output D
struct HeunBufs { size_t x, xn, d, x32, D, total; };
// a sampler's own buffers go behind the five: each take appends one, 256-byte aligned
static inline size_t heun_take(HeunBufs& b, size_t bytes) { size_t o = b.total; b.total += align_up(bytes, 256); return o; }
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

// (the samplers' other entry checks are one statement each, in an order and with texts of their own: they stay with them)
static inline int heun_check_workspace(const char* who, size_t have, size_t need) {
  if (need > have) {
    set_error("%s: workspace too small (%zu < %zu bytes)", who, have, need);
    return MCEDM_ERR_WORKSPACE;
  }
  return MCEDM_OK;
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

}  // namespace mcedm
