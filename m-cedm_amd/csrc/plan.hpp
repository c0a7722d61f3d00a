// plan.hpp -- host-side description of the network (block list, parameter table, packed-weight
// layout) and of the activation layout inside the caller's workspace.
#pragma once
#include <algorithm>
#include <initializer_list>
#include <string>
#include <utility>
#include <vector>

#include "common.hpp"

namespace mcedm {

constexpr size_t NONE = (size_t)-1;

// first-fit pool over the caller's workspace, simulated on the host (offsets only)
struct Pool {
  std::vector<std::pair<size_t, size_t>> free_;   // (offset, bytes), sorted by offset
  size_t top = 0, peak = 0;
  bool keep_all = false;
  size_t alloc(size_t bytes) {
    bytes = align_up(bytes ? bytes : 1, 256);
    for (size_t i = 0; i < free_.size(); ++i)
      if (free_[i].second >= bytes) {
        const size_t off = free_[i].first;
        if (free_[i].second == bytes) free_.erase(free_.begin() + i);
        else { free_[i].first += bytes; free_[i].second -= bytes; }
        return off;
      }
    const size_t off = top;
    top += bytes;
    peak = std::max(peak, top);
    return off;
  }
  void release(size_t off, size_t bytes) {
    if (keep_all) return;
    bytes = align_up(bytes ? bytes : 1, 256);
    auto it = std::lower_bound(free_.begin(), free_.end(), std::make_pair(off, (size_t)0));
    it = free_.insert(it, {off, bytes});
    if (it + 1 != free_.end() && it->first + it->second == (it + 1)->first) { it->second += (it + 1)->second; free_.erase(it + 1); }
    if (it != free_.begin() && (it - 1)->first + (it - 1)->second == it->first) { (it - 1)->second += it->second; it = free_.erase(it) - 1; }
    if (it->first + it->second == top) { top = it->first; free_.erase(it); }
  }
};

struct ParamInfo {
  std::string name;
  int ndim = 0;
  int64_t shape[4] = {1, 1, 1, 1};
  int64_t numel = 0;
};

// the parameter table of a plan, in state_dict order: append one entry, return its index
static inline int add_param(std::vector<ParamInfo>& params, const std::string& name, std::initializer_list<int64_t> shape) {
  ParamInfo pi;
  pi.name = name;
  pi.ndim = (int)shape.size();
  pi.numel = 1;
  int i = 0;
  for (int64_t s : shape) { pi.shape[i++] = s; pi.numel *= s; }
  params.push_back(pi);
  return (int)params.size() - 1;
}

static inline bool in_list(const int32_t* v, int n, int x) {
  for (int i = 0; i < n; ++i) if (v[i] == x) return true;
  return false;
}

// cursor over the packed-weight buffer (float offsets, 64-float granules)
struct Taker {
  size_t cur = 0;
  size_t take(size_t nfloats) { size_t o = cur; cur += align_up(nfloats, 64); return o; }
};

// The accessors both plan types export (mcedm_unet_* / mcedm_ddpm_*): PlanT has params, packed_floats and variants;
// `who` is the entry's name in its error texts.
template <class PlanT>
int plan_param_count(const PlanT* plan) { return plan ? (int)plan->params.size() : MCEDM_ERR_INVALID; }

template <class PlanT>
int plan_param_info(const PlanT* plan, const char* who, int index, const char** name, int64_t* numel, int32_t* ndim,
                    int64_t shape[4]) {
  MCEDM_REQUIRE(plan && index >= 0 && index < (int)plan->params.size(), "%s: index %d out of range", who, index);
  const ParamInfo& p = plan->params[index];
  if (name) *name = p.name.c_str();
  if (numel) *numel = p.numel;
  if (ndim) *ndim = p.ndim;
  if (shape) for (int i = 0; i < 4; ++i) shape[i] = p.shape[i];
  return MCEDM_OK;
}

template <class PlanT>
int plan_packed_bytes(const PlanT* plan, const char* who, size_t* bytes) {
  VariantScope variant_scope__(plan);
  MCEDM_REQUIRE(plan && bytes, "%s: null argument", who);
  *bytes = plan->packed_floats * sizeof(float);
  return MCEDM_OK;
}

template <class PlanT>
int plan_set_variant(PlanT* plan, const char* who, int which, int value) {
  MCEDM_REQUIRE(plan, "%s: null plan", who);
  MCEDM_REQUIRE(which >= 0 && which < KV_COUNT, "%s: unknown switch %d", who, which);
  MCEDM_REQUIRE(value >= -1 && value <= 1, "%s: value must be -1 (process default), 0 or 1", who);
  plan->variants.v[which] = value;
  return MCEDM_OK;
}

struct ConvP {   // one Conv2d with weights
  int w = -1, b = -1;          // parameter indices
  int cin = 0, cout = 0, taps = 0;
  int qkv_heads = 0;           // > 0: output rows re-ordered to (head, {q,k,v}, c)
  size_t wpk = NONE, bias = NONE;      // float offsets into the packed buffer
  size_t wpk_dgrad = NONE;             // transposed + mirrored weights for the data gradient
  size_t wino = NONE, wino_dgrad = NONE;   // both again in Winograd F(2x2, 3x3) form (conv_wino.hip) where that kernel can serve
  size_t wfrag = NONE;                 // a 1x1 skip projection's weights in MFMA-fragment order (ConvArgs::sk_wfrag) where conv1 may fold it
};

struct NormP {
  int w = -1, b = -1;
  int C = 0, groups = 0;
  size_t gamma = NONE, beta = NONE;    // float offsets into the packed buffer
};

struct BlockP {
  std::string key;
  int cin = 0, cout = 0;
  bool up = false, down = false, attn = false;
  int heads = 0;
  int skip_kernel = -1;        // -1 none (identity), 0 resample only, 1 1x1 conv
  NormP norm0, norm1, norm2;
  ConvP conv0, conv1, skip, qkv, proj;
  int aff_w = -1, aff_b = -1;
  int film_row0 = 0;           // first row of this block's (scale|shift) in the film table
};

// a tensor inside the workspace
struct TRef {
  size_t off = NONE;           // byte offset
  int C = 0, H = 0, W = 0;
  size_t bytes = 0;
  size_t sums = NONE;          // byte offset of the fused GroupNorm per-tile (sum, sumsq) table of this tensor, if any
  int sum_tiles = 0;           // tiles per sample the producing conv used (filled while the forward is scheduled)
  int ref = 0;                 // live references while the layout is being simulated
};

struct BlockLayout {
  int xa = -1, xb = -1;        // input tensor ids (xb = popped skip for concat blocks)
  int coef0 = -1, h = -1, coef1 = -1, sk = -1, y = -1, coef2 = -1, qkv = -1, a = -1, z = -1;
  int stats0 = -1, stats1 = -1, stats2 = -1;
  int xd = -1;                 // down blocks: the activated, 2x2-averaged input of conv0 (temporary)
  int out = -1;                // y or z
  int xd1 = -1;                // dropout (training, plan->dropout_p > 0): conv1's materialised input mask * s * silu(film(norm1(h)))
  int draw = 0;                // 0-based position in the order the blocks run (enc then dec): the draw index of the block's mask
  int wfold = 0;               // conv1 (Winograd kernel, SKIP variant) computes the 1x1 skip projection itself; `sk` stays reserved
  int Hin = 0, Win = 0, H = 0, W = 0;
};

struct Layout {
  std::vector<TRef> t;         // all tensors
  std::vector<BlockLayout> blocks;   // encoder blocks then decoder blocks
  int film = -1, t0 = -1, coef_out = -1, stats_out = -1, last = -1;
  // dx_cond head (adm_blocks.py:334-362): cat(x, dx) staging buffer (MCEDM_DX_CAT); conv_in output, dx_enc.0 output, its
  // GELU, dx_enc.2 output in front of combine_enc, whose output is then t0 (MCEDM_DX_ENC)
  int xdx = -1, xf = -1, d1 = -1, g1 = -1, d2 = -1;
  size_t sums_base = 0, sums_bytes = 0;   // arena of all fused-statistics tables
  size_t total_bytes = 0;
  bool training = false;       // laid out for training (build_layout)
  int seed = -1;               // dropout: the 8-byte seed the forward used, kept for the backward (behind every other tensor)
};

}  // namespace mcedm

struct mcedm_plan {
  mcedm_unet_desc desc;
  std::vector<mcedm::ParamInfo> params;
  mcedm::ConvP conv_in, conv_out;
  mcedm::ConvP dx_enc0, dx_enc2, combine;      // MCEDM_DX_ENC only (adm_blocks.py:266-280)
  mcedm::NormP out_norm;
  std::vector<mcedm::BlockP> enc, dec;
  int map0_w = -1, map0_b = -1, map1_w = -1, map1_b = -1;
  // packed buffer (float offsets)
  size_t freqs = mcedm::NONE, w0 = mcedm::NONE, b0 = mcedm::NONE, w1 = mcedm::NONE, b1 = mcedm::NONE;
  size_t waff = mcedm::NONE, baff = mcedm::NONE;
  int film_rows = 0;
  size_t packed_floats = 0;
  int levels_div = 1;          // 2^(n_levels-1)
  mcedm::KernelVariants variants;   // per-plan kernel choices (mcedm_unet_plan_set_variant); -1 = process default
  // training-step dropout (mcedm_unet_plan_set_dropout): probability, 0 = off, and the DEVICE address of the 64-bit seed
  double dropout_p = 0.0;
  const unsigned long long* dropout_seed = nullptr;
};

namespace mcedm {
int build_layout(const mcedm_plan& P, int B, int H, int W, int training, int n_noise, Layout* out);

// header in front of the U-Net activations: EDM coefficient rows, conv_in transform, F / F_uncond
struct Header {
  size_t coefs4, c_noise, coef_in, F, Fu, total;
};
Header header_for(const mcedm_plan& P, int B, int H, int W);

template <class T>
static inline T* at(void* ws, size_t off) { return reinterpret_cast<T*>(reinterpret_cast<char*>(ws) + off); }

// the one text of a workspace that is too small, for every entry of either network; `who` names the entry
static inline int heun_check_workspace(const char* who, size_t have, size_t need) {
  if (need > have) {
    set_error("%s: workspace too small (%zu < %zu bytes)", who, have, need);
    return MCEDM_ERR_WORKSPACE;
  }
  return MCEDM_OK;
}

// One evaluation's inputs: conv_in reads cat(cond, x[, dx]) scaled by the rows of coef_in (null = identity); cond and dx are
// optional (null: None).
struct AdmIn {
  const float* x = nullptr;
  const float* dx = nullptr;
  const float* cond = nullptr;
  const Coef* coef_in = nullptr;
  const float* noise_labels = nullptr;
};

// A plan bound to its packed weights, its region of a workspace (header, then activations), a shape and a stream.  The
// schedule and the header's offsets are plan.hip's; the samplers (sampler.hip) and the backward (backward.hip) go through
// the members.
struct AdmNet {
  const mcedm_plan* plan = nullptr;
  const float* pk = nullptr;
  Layout L;
  Header hd{};
  char* ws = nullptr;          // start of the network's region (its header)
  char* act = nullptr;         // start of the activations behind the header
  int B = 0, H = 0, W = 0, n_noise = 0;
  hipStream_t s = nullptr;

  int coef_batch() const { return n_noise > 1 ? 1 : 0; }      // per-sample rows (film, coef_in) with one label per sample
  bool dropout() const { return L.seed >= 0; }                // this layout carries the dropout tensors (training, p > 0)
  const unsigned long long* seed_slot() const { return reinterpret_cast<const unsigned long long*>(act + L.t[L.seed].off); }
  float* T(int id) const { return id < 0 ? nullptr : reinterpret_cast<float*>(act + L.t[id].off); }
  Coef* CF(int id) const { return id < 0 ? nullptr : reinterpret_cast<Coef*>(act + L.t[id].off); }
  float* SUMS(int id) const { return (id < 0 || L.t[id].sums == NONE) ? nullptr : reinterpret_cast<float*>(act + L.t[id].sums); }
  const float* film() const { return T(L.film); }
  // the header: network output with and without its conditioning, conv_in's rows, the noise labels and the EDM (c_skip, c_out, ..) rows
  float* F() const;
  float* Fu() const;
  Coef* coef_in() const;
  float* c_noise() const;
  float* coefs4() const;

  void place(const void* packed, void* region, void* stream);
  // one conv of the schedule: weights `cv`, sources xa | xb at Hs x Ws, output tensor `dst` at H x W with that tensor's
  // fused-statistics table if it has one (dst < 0: the caller sets `out`)
  ConvArgs conv(const ConvP& cv, const float* xa, int Ca, const float* xb, int Cb, int Hs, int Ws, int H, int W, int dst,
                std::vector<SumTiles>& st) const;
  int run_block(const BlockP& b, const BlockLayout& bl, std::vector<SumTiles>& st) const;
  int forward(const AdmIn& in, float* out) const;
  // F <- the network on `in`; Fu (unless null) <- the same without cond and dx: the two passes of classifier-free guidance
  int forward_cfg(AdmIn in, float* F, float* Fu) const {
    const int rc = forward(in, F);
    if (rc || !Fu) return rc;
    in.cond = in.dx = nullptr;
    return forward(in, Fu);
  }
};

// *net <- (P, shape, layout, header offsets), *bytes <- what the network needs of a workspace: header + activations.
// Three facts about who lays out how: the size queries lay out with n_noise = B; the samplers with n_noise = 1 and
// training = 0; mcedm_unet_forward_dx and mcedm_edm_denoise_dx with their own n_noise / n_sigma and their training flag, and
// they check header + activations only, not the backward's scratch (which the training size query adds and the backward checks).
int adm_sizes(const mcedm_plan& P, int B, int H, int W, int training, int n_noise, AdmNet* net, size_t* bytes);

// The one place that knows the workspace layout: `front_bytes` of the caller's own buffers (a sampler's), then the network's
// header and activations, then extra_bytes(net) of the caller's behind them (the backward's scratch, sized from the layout).
template <class Extra>
static inline int adm_bind(const char* who, const mcedm_plan& P, const void* packed, void* workspace, size_t workspace_bytes,
                           size_t front_bytes, Extra&& extra_bytes, int B, int H, int W, int training, int n_noise, void* stream,
                           AdmNet* net) {
  int rc;
  size_t need = 0;
  if ((rc = adm_sizes(P, B, H, W, training, n_noise, net, &need))) return rc;
  if ((rc = heun_check_workspace(who, workspace_bytes, front_bytes + need + extra_bytes(*net)))) return rc;
  net->place(packed, at<char>(workspace, front_bytes), stream);
  return MCEDM_OK;
}
static inline size_t no_extra(const AdmNet&) { return 0; }

// D = c_skip x + c_out F(c_in x; ln(sigma)/4; cond) with sigma from the device (net.n_noise rows) or, null, from the host
int denoise_impl(const AdmNet& net, const float* x, const float* dx, const float* cond, const float* sigma_dev, float sigma_host,
                 double w, float sigma_data, float* D_out, float* F_out);

// bytes the backward needs behind the training-mode activations (gradient buffers + scratch)
size_t backward_scratch_bytes(const mcedm_plan& P, const Layout& L, int B, int H, int W);
}
