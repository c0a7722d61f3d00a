// plan.hip -- the C ABI: plan construction, weight packing, workspace layout, the U-Net forward
// schedule and EDM denoise (the samplers on top of them: sampler.hip).  Host code only launches the kernels of
// conv_mfma.hip / norm_emb_attn.hip / edm.hip on the caller's stream; it never allocates device
// memory and never synchronises.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "edm.hpp"
#include "pack.hpp"
#include "plan.hpp"
#include "prof.hpp"
#include "bwd.hpp"

namespace mcedm {

static thread_local char g_err[1024] = "";

void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

// ------------------------------------------------------------------------------------------
// plan construction: restates DhariwalUNet.__init__ (models/adm_blocks.py:203-317)
// ------------------------------------------------------------------------------------------
static NormP make_norm(mcedm_plan& P, const std::string& key, int C) {
  NormP n;
  n.C = C;
  n.groups = std::min(32, C / 4);          // adm_blocks.py:89
  n.w = add_param(P.params, key + ".weight", {C});
  n.b = add_param(P.params, key + ".bias", {C});
  return n;
}

static ConvP make_conv(mcedm_plan& P, const std::string& key, int cin, int cout, int k, int qkv_heads = 0) {
  ConvP c;
  c.cin = cin; c.cout = cout; c.taps = k * k; c.qkv_heads = qkv_heads;
  c.w = add_param(P.params, key + ".weight", {cout, cin, k, k});
  c.b = add_param(P.params, key + ".bias", {cout});
  return c;
}

static BlockP make_block(mcedm_plan& P, const std::string& key, int cin, int cout, bool up, bool down, bool attn) {
  const int emb = P.desc.ch;
  BlockP b;
  b.key = key; b.cin = cin; b.cout = cout; b.up = up; b.down = down;
  b.heads = attn ? cout / P.desc.channels_per_head : 0;      // adm_blocks.py:135
  b.attn = b.heads > 0;
  b.norm0 = make_norm(P, key + ".norm0", cin);
  b.conv0 = make_conv(P, key + ".conv0", cin, cout, 3);
  b.aff_w = add_param(P.params, key + ".affine.weight", {2 * cout, emb});
  b.aff_b = add_param(P.params, key + ".affine.bias", {2 * cout});
  b.norm1 = make_norm(P, key + ".norm1", cout);
  b.conv1 = make_conv(P, key + ".conv1", cout, cout, 3);
  b.skip_kernel = -1;
  if (cout != cin || up || down) {                           // adm_blocks.py:148-151
    b.skip_kernel = (cout != cin) ? 1 : 0;
    if (b.skip_kernel == 1) b.skip = make_conv(P, key + ".skip", cin, cout, 1);
  }
  if (b.attn) {
    b.norm2 = make_norm(P, key + ".norm2", cout);
    b.qkv = make_conv(P, key + ".qkv", cout, 3 * cout, 1, b.heads);
    b.proj = make_conv(P, key + ".proj", cout, cout, 1);
  }
  return b;
}

static void place_conv(Taker& t, ConvP& c, bool dgrad) {
  c.wpk = t.take(conv_packed_floats(c.cout, c.cin, c.taps));
  c.bias = t.take((size_t)(c.cout + 31) / 32 * 32);
  if (dgrad) c.wpk_dgrad = t.take(conv_packed_floats(c.cin, c.cout, c.taps));
  if (c.taps == 9 && c.qkv_heads == 0) {       // Winograd tables where the kernel's channel constraints can be met
    // (whole 32-channel blocks: the split variant of the kernel, which serves the images below 32 x 32; the others need 64)
    if (c.cout % 32 == 0 && c.cin % 8 == 0) c.wino = t.take(conv_wino_packed_floats(c.cout, c.cin));
    if (dgrad && c.cin % 64 == 0 && c.cout % 8 == 0) c.wino_dgrad = t.take(conv_wino_packed_floats(c.cin, c.cout));
  }
}
// a skip projection that the Winograd kernel's SKIP variant can compute in conv1's epilogue (conv_wino.hip): fragment order
static void place_skip_frag(Taker& t, ConvP& c) {
  if (c.taps == 1 && c.cout % 128 == 0 && c.cin % 16 == 0 && c.cin >= 32 && c.cin <= 256) c.wfrag = t.take(conv_frag_packed_floats(c.cout, c.cin));
}
static void place_norm(Taker& t, NormP& n) { n.gamma = t.take(n.C); n.beta = t.take(n.C); }

}  // namespace mcedm

using namespace mcedm;

extern "C" int mcedm_version(void) { return MCEDM_ABI_VERSION; }

extern "C" int mcedm_unet_plan_set_variant(mcedm_plan* plan, int which, int value) {
  return plan_set_variant(plan, "plan_set_variant", which, value);
}
extern "C" int mcedm_unet_plan_set_dropout(mcedm_plan* plan, double p, const uint64_t* rng_seed) {
  MCEDM_REQUIRE(plan, "plan_set_dropout: null plan");
  MCEDM_REQUIRE(p >= 0.0 && (float)p < 1.0f, "plan_set_dropout: p=%g must lie in [0, 1)", p);      // (NaN fails the first test)
  MCEDM_REQUIRE(p == 0.0 || rng_seed, "plan_set_dropout: p=%g > 0 needs the device address of a seed", p);
  plan->dropout_p = p;
  plan->dropout_seed = p > 0.0 ? reinterpret_cast<const unsigned long long*>(rng_seed) : nullptr;
  return MCEDM_OK;
}
extern "C" const char* mcedm_last_error(void) { return g_err; }

extern "C" int mcedm_unet_plan_create(const mcedm_unet_desc* d, mcedm_plan** out) {
  MCEDM_REQUIRE(d && out, "plan_create: null argument");
  MCEDM_REQUIRE(d->n_levels >= 1 && d->n_levels <= MCEDM_MAX_LEVELS, "plan_create: n_levels=%d out of range", d->n_levels);
  MCEDM_REQUIRE(d->n_attn_resolutions >= 0 && d->n_attn_resolutions <= MCEDM_MAX_LEVELS, "plan_create: bad n_attn_resolutions");
  MCEDM_REQUIRE(d->in_channels > 0 && d->out_channels > 0 && d->cond_channels >= 0, "plan_create: bad channel counts");
  MCEDM_REQUIRE(d->ch > 0 && d->ch % 8 == 0, "plan_create: ch=%d must be a positive multiple of 8", d->ch);
  MCEDM_REQUIRE(d->num_res_blocks >= 1, "plan_create: num_res_blocks must be >= 1");
  if (d->channels_per_head != 64) {
    set_error("plan_create: channels_per_head=%d unsupported (the hot path uses 64, adm_blocks.py:223)", d->channels_per_head);
    return MCEDM_ERR_UNSUPPORTED;
  }
  for (int l = 0; l < d->n_levels; ++l) {
    const int c = d->ch * d->ch_mult[l];
    MCEDM_REQUIRE(d->ch_mult[l] >= 1 && c % 8 == 0, "plan_create: level %d width %d must be a multiple of 8", l, c);
  }
  MCEDM_REQUIRE(d->dx_mode == MCEDM_DX_NONE || d->dx_mode == MCEDM_DX_CAT || d->dx_mode == MCEDM_DX_ENC, "plan_create: dx_mode=%d", d->dx_mode);
  MCEDM_REQUIRE((d->dx_mode == MCEDM_DX_NONE) == (d->dx_channels == 0) && d->dx_channels >= 0,
                "plan_create: dx_channels=%d does not go with dx_mode=%d", d->dx_channels, d->dx_mode);
  mcedm_plan* Pp = new mcedm_plan();
  mcedm_plan& P = *Pp;
  P.desc = *d;
  P.levels_div = 1 << (d->n_levels - 1);
  const int ch = d->ch;
  auto key = [&](const char* side, int res, const std::string& tail) {
    return std::string(side) + "." + std::to_string(res) + "x" + std::to_string(res) + "_" + tail;
  };
  P.map0_w = add_param(P.params, "map_layer0.weight", {ch, ch});
  P.map0_b = add_param(P.params, "map_layer0.bias", {ch});
  P.map1_w = add_param(P.params, "map_layer1.weight", {ch, ch});
  P.map1_b = add_param(P.params, "map_layer1.bias", {ch});
  if (d->dx_mode == MCEDM_DX_ENC) {        // registered before self.enc (adm_blocks.py:266-280): state_dict order
    const int c0 = ch * d->ch_mult[0];
    P.dx_enc0 = make_conv(P, "dx_enc.0", d->dx_channels, c0, 3);
    P.dx_enc2 = make_conv(P, "dx_enc.2", c0, c0, 3);
    P.combine = make_conv(P, "combine_enc", 2 * c0, c0, 3);
  }
  std::vector<int> skips;
  int cout = d->in_channels + d->cond_channels + (d->dx_mode == MCEDM_DX_CAT ? d->dx_channels : 0);   // adm_blocks.py:236-238
  for (int level = 0; level < d->n_levels; ++level) {
    const int res = d->resolution >> level, mult = d->ch_mult[level];
    if (level == 0) {
      const int cin = cout;
      cout = ch * mult;
      P.conv_in = make_conv(P, key("enc", res, "conv"), cin, cout, 3);
      skips.push_back(cout);
    } else {
      P.enc.push_back(make_block(P, key("enc", res, "down"), cout, cout, false, true, false));
      skips.push_back(cout);
    }
    for (int idx = 0; idx < d->num_res_blocks; ++idx) {
      const int cin = cout;
      cout = ch * mult;
      const bool attn = in_list(d->attn_resolutions, d->n_attn_resolutions, res);
      P.enc.push_back(make_block(P, key("enc", res, "block" + std::to_string(idx)), cin, cout, false, false, attn));
      skips.push_back(cout);
    }
  }
  for (int level = d->n_levels - 1; level >= 0; --level) {
    const int res = d->resolution >> level, mult = d->ch_mult[level];
    if (level == d->n_levels - 1) {
      P.dec.push_back(make_block(P, key("dec", res, "in0"), cout, cout, false, false, true));
      P.dec.push_back(make_block(P, key("dec", res, "in1"), cout, cout, false, false, false));
    } else {
      P.dec.push_back(make_block(P, key("dec", res, "up"), cout, cout, true, false, false));
    }
    for (int idx = 0; idx < d->num_res_blocks + 1; ++idx) {
      const int cin = cout + skips.back();
      skips.pop_back();
      cout = ch * mult;
      const bool attn = in_list(d->attn_resolutions, d->n_attn_resolutions, res);
      P.dec.push_back(make_block(P, key("dec", res, "block" + std::to_string(idx)), cin, cout, false, false, attn));
    }
  }
  P.out_norm = make_norm(P, "out_norm", cout);
  P.conv_out = make_conv(P, "out_conv", cout, d->out_channels, 3);
  // the attention kernels are built for head_dim == 64; the reference's head_dim is cout / (cout // 64)
  // (adm_blocks.py:135,175), which differs as soon as cout is not a multiple of 64 (e.g. 96 -> one head of 96)
  for (auto* v : {&P.enc, &P.dec})
    for (const BlockP& b : *v)
      if (b.attn && b.cout % d->channels_per_head != 0) {
        set_error("plan_create: block %s has attention with %d channels, not a multiple of channels_per_head=%d "
                  "(head_dim %d is not built)", b.key.c_str(), b.cout, d->channels_per_head, b.cout / b.heads);
        delete Pp;
        return MCEDM_ERR_UNSUPPORTED;
      }
  // GroupNorm(C) has min(32, C / 4) groups (adm_blocks.py:89), which must divide C: a width or a concat of 128 channels or more
  // that is not a multiple of 32 (144 = 96 + 48) is no network of the reference's either, and is refused here, not at the first forward
  {
    std::vector<std::pair<std::string, const NormP*>> norms;
    for (auto* v : {&P.enc, &P.dec})
      for (const BlockP& b : *v) {
        norms.push_back({b.key + ".norm0", &b.norm0});
        norms.push_back({b.key + ".norm1", &b.norm1});
        if (b.attn) norms.push_back({b.key + ".norm2", &b.norm2});
      }
    norms.push_back({"out_norm", &P.out_norm});
    for (const auto& kn : norms)
      if (kn.second->groups <= 0 || kn.second->C % kn.second->groups != 0) {
        set_error("plan_create: GroupNorm %s has %d channels, not a multiple of its %d groups (min(32, C / 4))", kn.first.c_str(),
                  kn.second->C, kn.second->groups);
        delete Pp;
        return MCEDM_ERR_UNSUPPORTED;
      }
  }

  // packed-buffer layout
  Taker t;
  P.freqs = t.take(ch / 2);
  P.w0 = t.take((size_t)ch * ch); P.b0 = t.take(ch);
  P.w1 = t.take((size_t)ch * ch); P.b1 = t.take(ch);
  int rows = 0;
  for (auto* v : {&P.enc, &P.dec})
    for (BlockP& b : *v) { b.film_row0 = rows; rows += 2 * b.cout; }
  P.film_rows = rows;
  P.waff = t.take((size_t)rows * ch);
  P.baff = t.take(rows);
  place_conv(t, P.conv_in, false);
  if (d->dx_mode == MCEDM_DX_ENC) { place_conv(t, P.dx_enc0, false); place_conv(t, P.dx_enc2, true); place_conv(t, P.combine, true); }
  for (auto* v : {&P.enc, &P.dec})
    for (BlockP& b : *v) {
      place_norm(t, b.norm0); place_conv(t, b.conv0, true);
      place_norm(t, b.norm1); place_conv(t, b.conv1, true);
      if (b.skip_kernel == 1) { place_conv(t, b.skip, true); if (!b.up && !b.down) place_skip_frag(t, b.skip); }
      if (b.attn) { place_norm(t, b.norm2); place_conv(t, b.qkv, true); place_conv(t, b.proj, true); }
    }
  place_norm(t, P.out_norm);
  place_conv(t, P.conv_out, true);
  P.packed_floats = t.cur;
  *out = Pp;
  return MCEDM_OK;
}

extern "C" void mcedm_unet_plan_destroy(mcedm_plan* plan) { delete plan; }

extern "C" int mcedm_unet_param_count(const mcedm_plan* plan) { return plan_param_count(plan); }

extern "C" int mcedm_unet_param_info(const mcedm_plan* plan, int index, const char** name, int64_t* numel, int32_t* ndim,
                                     int64_t shape[4]) {
  return plan_param_info(plan, "param_info", index, name, numel, ndim, shape);
}

extern "C" int mcedm_unet_packed_bytes(const mcedm_plan* plan, size_t* bytes) {
  return plan_packed_bytes(plan, "packed_bytes", bytes);
}

// ------------------------------------------------------------------------------------------
// weight packing
// ------------------------------------------------------------------------------------------
namespace mcedm {

constexpr int COPY_MAX = 40;
struct CopyBatch {
  const float* src[COPY_MAX];
  float* dst[COPY_MAX];
  int n[COPY_MAX];
};

__global__ void batched_copy_kernel(CopyBatch b) {
  const int j = blockIdx.y;
  const float* s = b.src[j];
  float* d = b.dst[j];
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < b.n[j]; i += gridDim.x * blockDim.x) d[i] = s[i];
}

// freqs[k] = (1/10000)^(k/half)   (adm_blocks.py:193-196, endpoint=False): the fp32 power of the fp32 operands, correctly rounded
// (evaluated in fp64).  The device's powf is 1 ulp off that for 7 of the 32 frequencies at ch = 64, where torch's CPU pow is not;
// at a DDPM label of ~1000 one ulp of a frequency is 3e-5 in cos / sin(t * freq) (500 ulp), which the gradient of
// map_layer0.weight shows at 1e-5 of its maximum.
__global__ void freqs_kernel(float* f, int half) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k < half) f[k] = (float)pow((double)(1.0f / 10000.0f), (double)((float)k / (float)half));
}

// Every conv weight of a plan is re-laid per optimisation step (direct form, its data-gradient mirror, both again in
// Winograd form): as one launch per table that was ~140 kernels of 4-5 us per training step (profiles/r3_train_kernel_stats.csv:
// 805 + 560 calls in six steps).  The jobs are batched instead: one launch packs up to PACK_MAX tables, a fixed number of
// workgroups per table walking its elements (pack.hpp holds the per-element bodies, shared with the one-table kernels).
constexpr int PACK_MAX = 48;
struct PackJob {
  const float* w; float* dst;
  int Cout, Cin, taps, KC, coutp, qkv_heads, tflip;
  int kind;                     // 0: direct form (pack_conv_value), 1: Winograd F(2x2, 3x3) form (wino_pack_elem), 2: fragment order (frag_pack_value)
  unsigned total;               // elements to walk: packed floats (direct) or coutp * nch * WKC (Winograd)
};
struct PackBatch { PackJob j[PACK_MAX]; };
static_assert(sizeof(PackBatch) <= 4000, "kernel argument budget");

__global__ void pack_batch_kernel(PackBatch b) {
  const PackJob& J = b.j[blockIdx.y];
  for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < J.total; i += gridDim.x * blockDim.x) {
    if (J.kind == 0) J.dst[i] = pack_conv_value(J.w, i, J.Cout, J.Cin, J.taps, J.KC, J.coutp, J.qkv_heads, J.tflip);
    else if (J.kind == 2) J.dst[i] = frag_pack_value(J.w, (int)i, J.Cout, J.Cin, J.coutp);
    else wino_pack_elem(J.w, J.dst, (int)i, J.Cout, J.Cin, J.coutp, J.tflip);
  }
}

struct Packer {
  PackBatch b;
  int count = 0;
  hipStream_t s;
  int status = MCEDM_OK;
  double bytes = 0.0;           // read + written by the batch (profiler row: an HBM-bound kernel)
  void flush() {
    if (count == 0 || status != MCEDM_OK) { count = 0; bytes = 0.0; return; }
    {
      ProfScope ps("pack_batch_kernel", 0.0, bytes, s);
      hipLaunchKernelGGL(pack_batch_kernel, dim3(48, count), dim3(256), 0, s, b);
      if (hipGetLastError() != hipSuccess) { set_error("pack_batch_kernel launch failed"); status = MCEDM_ERR_HIP; }
    }
    count = 0; bytes = 0.0;
  }
  void add(const PackJob& j) {
    b.j[count] = j;
    // direct tables: one float read per float written; Winograd: 9 taps read, 16 positions written per (cout, cin)
    bytes += j.kind != 1 ? 8.0 * j.total : 4.0 * (9.0 + 16.0) * j.total;
    if (++count == PACK_MAX) flush();
  }
  void conv(const float* w, float* dst, int Cout, int Cin, int taps, int qkv_heads, int tflip) {
    const size_t total = conv_packed_floats(Cout, Cin, taps);
    if (total >= (1ull << 32)) { set_error("pack: table too large"); status = MCEDM_ERR_INVALID; return; }
    add(PackJob{w, dst, Cout, Cin, taps, conv_kc_for(taps), cout_padded(Cout), qkv_heads, tflip, 0, (unsigned)total});
  }
  void frag(const float* w, float* dst, int Cout, int Cin) {
    add(PackJob{w, dst, Cout, Cin, 1, 8, cout_padded(Cout), 0, 0, 2, (unsigned)conv_frag_packed_floats(Cout, Cin)});
  }
  void wino(const float* w, float* dst, int Cout, int Cin, int tflip) {
    const int coutp = cout_padded(Cout), nch = ceil_div(Cin, WKC);
    add(PackJob{w, dst, Cout, Cin, 9, WKC, coutp, 0, tflip, 1, (unsigned)(coutp * nch * WKC)});
  }
};

struct Copier {
  CopyBatch b;
  int count = 0;
  hipStream_t s;
  int status = MCEDM_OK;
  void flush() {
    if (count == 0 || status != MCEDM_OK) { count = 0; return; }
    hipLaunchKernelGGL(batched_copy_kernel, dim3(8, count), dim3(256), 0, s, b);
    if (hipGetLastError() != hipSuccess) { set_error("batched_copy_kernel launch failed"); status = MCEDM_ERR_HIP; }
    count = 0;
  }
  void add(const float* src, float* dst, size_t n) {
    b.src[count] = src; b.dst[count] = dst; b.n[count] = (int)n;
    if (++count == COPY_MAX) flush();
  }
};

static int pack_conv(const ConvP& c, const float* const* params, float* pk, Copier& cp, Packer& pp, hipStream_t s) {
  pp.conv(params[c.w], pk + c.wpk, c.cout, c.cin, c.taps, c.qkv_heads, 0);
  int rc = MCEDM_OK;
  if (c.qkv_heads > 0) rc = launch_pack_bias(params[c.b], pk + c.bias, c.cout, c.qkv_heads, s);
  else cp.add(params[c.b], pk + c.bias, c.cout);
  if (rc) return rc;
  // data-gradient GEMM: output channels = conv input channels; for the qkv conv the K index follows the packed
  // (head, which, c) order of the incoming gradient rows
  if (c.wpk_dgrad != NONE) pp.conv(params[c.w], pk + c.wpk_dgrad, c.cin, c.cout, c.taps, c.qkv_heads, 1);
  if (c.wino != NONE) pp.wino(params[c.w], pk + c.wino, c.cout, c.cin, 0);
  if (c.wino_dgrad != NONE) pp.wino(params[c.w], pk + c.wino_dgrad, c.cin, c.cout, 1);
  if (c.wfrag != NONE) pp.frag(params[c.w], pk + c.wfrag, c.cout, c.cin);
  return pp.status;
}

static void pack_norm(const NormP& n, const float* const* params, float* pk, Copier& cp) {
  cp.add(params[n.w], pk + n.gamma, n.C);
  cp.add(params[n.b], pk + n.beta, n.C);
}

}  // namespace mcedm

extern "C" int mcedm_unet_pack_weights(const mcedm_plan* plan, const float* const* params, void* packed, void* stream) {
  VariantScope variant_scope__(plan);
  MCEDM_REQUIRE(plan && params && packed, "pack_weights: null argument");
  const mcedm_plan& P = *plan;
  for (size_t i = 0; i < P.params.size(); ++i)
    MCEDM_REQUIRE(params[i] != nullptr, "pack_weights: parameter %zu (%s) is null", i, P.params[i].name.c_str());
  hipStream_t s = (hipStream_t)stream;
  float* pk = (float*)packed;
  const int ch = P.desc.ch;
  hipLaunchKernelGGL(freqs_kernel, dim3(ceil_div(ch / 2, 64)), dim3(64), 0, s, pk + P.freqs, ch / 2);
  MCEDM_LAUNCH_CHECK("freqs_kernel");
  Copier cp;
  cp.s = s;
  Packer pp;
  pp.s = s;
  cp.add(params[P.map0_w], pk + P.w0, (size_t)ch * ch); cp.add(params[P.map0_b], pk + P.b0, ch);
  cp.add(params[P.map1_w], pk + P.w1, (size_t)ch * ch); cp.add(params[P.map1_b], pk + P.b1, ch);
  int rc = pack_conv(P.conv_in, params, pk, cp, pp, s);
  if (rc) return rc;
  if (P.desc.dx_mode == MCEDM_DX_ENC) {
    if ((rc = pack_conv(P.dx_enc0, params, pk, cp, pp, s))) return rc;
    if ((rc = pack_conv(P.dx_enc2, params, pk, cp, pp, s))) return rc;
    if ((rc = pack_conv(P.combine, params, pk, cp, pp, s))) return rc;
  }
  for (auto* v : {&P.enc, &P.dec})
    for (const BlockP& b : *v) {
      cp.add(params[b.aff_w], pk + P.waff + (size_t)b.film_row0 * ch, (size_t)2 * b.cout * ch);
      cp.add(params[b.aff_b], pk + P.baff + b.film_row0, (size_t)2 * b.cout);
      pack_norm(b.norm0, params, pk, cp);
      pack_norm(b.norm1, params, pk, cp);
      if ((rc = pack_conv(b.conv0, params, pk, cp, pp, s))) return rc;
      if ((rc = pack_conv(b.conv1, params, pk, cp, pp, s))) return rc;
      if (b.skip_kernel == 1 && (rc = pack_conv(b.skip, params, pk, cp, pp, s))) return rc;
      if (b.attn) {
        pack_norm(b.norm2, params, pk, cp);
        if ((rc = pack_conv(b.qkv, params, pk, cp, pp, s))) return rc;
        if ((rc = pack_conv(b.proj, params, pk, cp, pp, s))) return rc;
      }
    }
  pack_norm(P.out_norm, params, pk, cp);
  if ((rc = pack_conv(P.conv_out, params, pk, cp, pp, s))) return rc;
  cp.flush();
  pp.flush();
  return cp.status != MCEDM_OK ? cp.status : pp.status;
}

// ------------------------------------------------------------------------------------------
// activation layout inside the workspace (first-fit pool, simulated on the host)
// ------------------------------------------------------------------------------------------
namespace mcedm {

struct LayoutBuilder {
  Layout& L;
  Pool pool;
  int B;
  int make(int C, int H, int W, size_t bytes) {
    TRef t;
    t.C = C; t.H = H; t.W = W; t.bytes = bytes;
    t.off = pool.alloc(bytes);
    L.t.push_back(t);
    return (int)L.t.size() - 1;
  }
  int act(int C, int H, int W) { return make(C, H, W, (size_t)B * C * H * W * sizeof(float)); }
  int coef(int C) { return make(C, 1, 1, (size_t)B * C * sizeof(Coef)); }
  int stats(int groups) { return make(groups, 1, 1, (size_t)B * groups * 2 * sizeof(float)); }
  void retain(int id) { if (id >= 0) L.t[id].ref++; }
  void release(int id) {
    if (id < 0) return;
    if (--L.t[id].ref == 0) pool.release(L.t[id].off, L.t[id].bytes);
  }
  void drop(int id) { if (id >= 0) pool.release(L.t[id].off, L.t[id].bytes); }   // un-refcounted temporaries
};

int build_layout(const mcedm_plan& P, int B, int H, int W, int training, int n_noise, Layout* out) {
  MCEDM_REQUIRE(B > 0 && H > 0 && W > 0, "layout: empty shape B=%d H=%d W=%d", B, H, W);
  MCEDM_REQUIRE(H % P.levels_div == 0 && W % P.levels_div == 0,
                "layout: H=%d W=%d must be multiples of %d (2^(levels-1))", H, W, P.levels_div);
  MCEDM_REQUIRE(n_noise == 1 || n_noise == B, "layout: n_noise=%d must be 1 or B=%d", n_noise, B);
  Layout& L = *out;
  L = Layout();
  L.training = training != 0;
  LayoutBuilder lb{L, Pool(), B};
  lb.pool.keep_all = training != 0;
  L.film = lb.make(P.film_rows, 1, 1, (size_t)n_noise * P.film_rows * sizeof(float));
  // arena of fused GroupNorm statistics: one [B][tiles][C/4][2] fp32 table per conv output that feeds a GroupNorm
  // (conv_in output, and h / y / z of every block), sized for the smallest pixel tile
  auto sums_sz = [&](int C, int h, int w) { return align_up((size_t)B * conv_max_tiles(h, w) * ceil_div(C, 4) * 2 * sizeof(float), 256); };
  {
    size_t need = sums_sz(P.conv_in.cout, H, W);
    int h = H, w = W;
    for (auto* v : {&P.enc, &P.dec})
      for (const BlockP& b : *v) {
        if (b.up) { h *= 2; w *= 2; } else if (b.down) { h /= 2; w /= 2; }
        need += (size_t)(b.attn ? 3 : 2) * sums_sz(b.cout, h, w);
      }
    L.sums_bytes = need;
    const int id = lb.make(1, 1, 1, need);
    L.sums_base = L.t[id].off;
  }
  size_t sums_cur = L.sums_base;
  auto give_sums = [&](int id) {
    L.t[id].sums = sums_cur;
    sums_cur += sums_sz(L.t[id].C, L.t[id].H, L.t[id].W);
  };
  if (P.desc.dx_mode == MCEDM_DX_CAT) L.xdx = lb.act(P.desc.in_channels + P.desc.dx_channels, H, W);
  if (P.desc.dx_mode == MCEDM_DX_ENC) {
    L.xf = lb.act(P.conv_in.cout, H, W);
    L.d1 = lb.act(P.conv_in.cout, H, W);
    L.g1 = lb.act(P.conv_in.cout, H, W);
    L.d2 = lb.act(P.conv_in.cout, H, W);
  }
  L.t0 = lb.act(P.conv_in.cout, H, W);
  give_sums(L.t0);
  lb.drop(L.xdx); lb.drop(L.xf); lb.drop(L.d1); lb.drop(L.g1); lb.drop(L.d2);      // the head's temporaries (kept in training)
  std::vector<int> skips;
  int cur = L.t0;
  lb.retain(cur);                 // chain reference
  lb.retain(cur); skips.push_back(cur);

  auto do_block = [&](const BlockP& b, int xa, int xb) {
    BlockLayout bl;
    bl.xa = xa; bl.xb = xb;
    bl.Hin = L.t[xa].H; bl.Win = L.t[xa].W;
    bl.H = b.up ? bl.Hin * 2 : (b.down ? bl.Hin / 2 : bl.Hin);
    bl.W = b.up ? bl.Win * 2 : (b.down ? bl.Win / 2 : bl.Win);
    bl.coef0 = lb.coef(b.cin);
    if (training) bl.stats0 = lb.stats(b.norm0.groups);
    // a down block's conv0 reads avgpool2x2(silu(norm(x))): four SiLUs per staged element is paid in matrix time
    // inside the fused kernel (62 vs 120 TFLOP/s), so that one input is materialised by an HBM-speed pass instead
    if (b.down) bl.xd = lb.act(b.cin, bl.H, bl.W);
    bl.h = lb.act(b.cout, bl.H, bl.W);
    give_sums(bl.h);
    lb.drop(bl.coef0); lb.drop(bl.xd);
    bl.coef1 = lb.coef(b.cout);
    if (training) bl.stats1 = lb.stats(b.norm1.groups);
    // the 1x1 skip projection is folded into conv1 (ConvArgs::sk_*) in inference AND in training: the backward never reads
    // the projected tensor (its weight gradient takes dy and the block input, its data gradient dy alone), so it only
    // exists for the resampling blocks, which the fold does not serve
    // ... and for blocks whose conv1 the Winograd kernel serves (conv_wino.hip): a 1x1 projection has nothing to gain
    // from that transform (it would cost 16 multiplies per output instead of 1), so it runs as its own launch there
    // and enters conv1 as a residual
    // ... unless that kernel's SKIP variant takes the projection into conv1's epilogue (inference only: training runs as before;
    // a choice by shape and channels, never by the batch).  The tensor stays RESERVED all the same: the workspace a caller sized
    // is then good for either path -- the fold can be switched per call (mcedm_op_set_conv_wino_fold, MCEDM_WINO_FOLD) without
    // laying the workspace out again -- and a plan's workspace_bytes is what it was
    const bool wino1 = b.conv1.wino != NONE && conv_wino_shape_ok(b.cout, b.cout, bl.H, bl.W);
    const bool wfold = wino1 && !training && !b.up && !b.down && b.skip_kernel == 1 && b.skip.wfrag != NONE &&
                       conv_wino_fold_shape_ok(b.cout, L.t[xa].C, xb >= 0 ? L.t[xb].C : 0, bl.H, bl.W);
    if (b.skip_kernel == 1 && (b.up || b.down || wino1)) bl.sk = lb.act(b.cout, bl.H, bl.W);
    bl.wfold = wfold ? 1 : 0;
    bl.y = lb.act(b.cout, bl.H, bl.W);
    give_sums(bl.y);
    lb.drop(bl.h); lb.drop(bl.coef1); lb.drop(bl.sk);
    bl.out = bl.y;
    if (b.attn) {
      bl.coef2 = lb.coef(b.cout);
      if (training) bl.stats2 = lb.stats(b.norm2.groups);
      bl.qkv = lb.act(3 * b.cout, bl.H, bl.W);
      lb.drop(bl.coef2);
      bl.a = lb.act(b.cout, bl.H, bl.W);
      lb.drop(bl.qkv);
      bl.z = lb.act(b.cout, bl.H, bl.W);
      give_sums(bl.z);
      lb.drop(bl.a); lb.drop(bl.y);
      bl.out = bl.z;
    }
    L.blocks.push_back(bl);
    return bl.out;
  };

  for (const BlockP& b : P.enc) {
    const int o = do_block(b, cur, -1);
    lb.retain(o);                 // chain
    lb.retain(o); skips.push_back(o);
    lb.release(cur);
    cur = o;
  }
  for (const BlockP& b : P.dec) {
    int xb = -1;
    if (L.t[cur].C != b.cin) {    // adm_blocks.py:400-401
      MCEDM_REQUIRE(!skips.empty(), "layout: skip stack underflow at %s", b.key.c_str());
      xb = skips.back(); skips.pop_back();
      MCEDM_REQUIRE(L.t[cur].C + L.t[xb].C == b.cin && L.t[cur].H == L.t[xb].H && L.t[cur].W == L.t[xb].W,
                    "layout: concat mismatch at %s", b.key.c_str());
    }
    const int o = do_block(b, cur, xb);
    lb.retain(o);
    lb.release(cur);
    lb.release(xb);
    cur = o;
  }
  L.last = cur;
  L.coef_out = lb.coef(P.out_norm.C);
  if (training) L.stats_out = lb.stats(P.out_norm.groups);
  // dropout (mcedm_unet_plan_set_dropout): every block's conv1 reads a materialised input, kept for its weight gradient, and the
  // backward finds the forward's seed in a slot of its own.  Behind every other tensor: with the plan's p = 0 nothing moves.
  if (training && P.dropout_p > 0.0) {
    size_t j = 0;
    for (auto* v : {&P.enc, &P.dec})
      for (const BlockP& b : *v) {
        BlockLayout& bl = L.blocks[j];
        bl.draw = (int)j++;
        bl.xd1 = lb.act(b.cout, bl.H, bl.W);
      }
    L.seed = lb.make(1, 1, 1, sizeof(unsigned long long));
  }
  L.total_bytes = lb.pool.peak;
  return MCEDM_OK;
}

// header in front of the U-Net activations: EDM coefficient rows, conv_in transform, F / F_uncond
Header header_for(const mcedm_plan& P, int B, int H, int W) {
  Header h;
  size_t cur = 0;
  auto take = [&](size_t bytes) { size_t o = cur; cur += align_up(bytes, 256); return o; };
  const int Ct = P.desc.in_channels + P.desc.cond_channels + P.desc.dx_channels;
  h.coefs4 = take((size_t)B * 4 * sizeof(float));
  h.c_noise = take((size_t)B * sizeof(float));
  h.coef_in = take((size_t)B * Ct * sizeof(Coef));
  h.F = take((size_t)B * P.desc.out_channels * H * W * sizeof(float));
  h.Fu = take((size_t)B * P.desc.out_channels * H * W * sizeof(float));
  h.total = cur;
  return h;
}

float* AdmNet::F() const { return at<float>(ws, hd.F); }
float* AdmNet::Fu() const { return at<float>(ws, hd.Fu); }
Coef* AdmNet::coef_in() const { return at<Coef>(ws, hd.coef_in); }
float* AdmNet::c_noise() const { return at<float>(ws, hd.c_noise); }
float* AdmNet::coefs4() const { return at<float>(ws, hd.coefs4); }

void AdmNet::place(const void* packed, void* region, void* stream) {
  pk = (const float*)packed; ws = (char*)region; act = ws + hd.total; s = (hipStream_t)stream;
}

int adm_sizes(const mcedm_plan& P, int B, int H, int W, int training, int n_noise, AdmNet* net, size_t* bytes) {
  const int rc = build_layout(P, B, H, W, training, n_noise, &net->L);
  if (rc) return rc;
  net->plan = &P; net->hd = header_for(P, B, H, W);
  net->B = B; net->H = H; net->W = W; net->n_noise = n_noise;
  *bytes = net->hd.total + net->L.total_bytes;
  return MCEDM_OK;
}

// ------------------------------------------------------------------------------------------
// forward schedule (adm_blocks.py:364-404 and :159-181)
// ------------------------------------------------------------------------------------------
// Inference: the consuming conv derives the GroupNorm(+FiLM) rows itself from the producers' partial sums
// (ConvArgs::gn_on), so no GroupNorm kernel is launched.  Training keeps the table (wgrad / GN backward read it and
// the saved statistics), as does any consumer that needs the table in memory (need_table) or a shape without
// usable partial sums.
static int gn_for_conv(const GnArgs& g, ConvArgs& c, bool need_table, hipStream_t s) {
  if (!need_table && g.stats == nullptr && gn_sums_usable(g)) {
    c.gn = g; c.gn_on = 1; c.coef = nullptr;
    return MCEDM_OK;
  }
  return launch_gn_coef_from_sums(g, s);
}

// One conv of the schedule.  The caller then sets only what is particular to it: coef / act / resample, res / res_mode, the
// sk_* fold fields.
ConvArgs AdmNet::conv(const ConvP& cv, const float* xa, int Ca, const float* xb, int Cb, int Hs, int Ws, int H, int W, int dst,
                      std::vector<SumTiles>& st) const {
  ConvArgs c{};
  c.xa = xa; c.Ca = Ca; c.xb = xb; c.Cb = Cb;
  c.Hs = Hs; c.Ws = Ws; c.H = H; c.W = W;
  c.wpk = pk + cv.wpk; c.bias = pk + cv.bias;
  // (training keeps the kernels its backward was built on: below 32 x 32 its convs carry no Winograd table, so the split variant never takes them)
  c.wino = cv.wino != NONE && !(L.training && conv_wino_small(H, W)) ? pk + cv.wino : nullptr;
  c.out = T(dst); c.Cout = cv.cout; c.B = B;
  c.gsum = SUMS(dst); c.gsum_tiles = c.gsum ? &st[dst] : nullptr;
  return c;
}

int AdmNet::run_block(const BlockP& b, const BlockLayout& bl, std::vector<SumTiles>& st) const {
  const mcedm_plan& P = *plan;
  auto TL = [&](int id) -> SumTiles { return id < 0 ? SumTiles{} : st[id]; };      // tiling of that tensor's statistics table
  const float* xa = T(bl.xa);
  const float* xb = T(bl.xb);
  const int Ca = L.t[bl.xa].C, Cb = bl.xb >= 0 ? L.t[bl.xb].C : 0;
  const float eps = P.desc.eps;
  int rc;
  // norm0 -> transform table for conv0
  GnArgs g0{xa, xb, Ca, Cb, bl.Hin * bl.Win, B, b.norm0.groups, pk + b.norm0.gamma, pk + b.norm0.beta,
            nullptr, 0, 0, eps, CF(bl.coef0), T(bl.stats0), SUMS(bl.xa), SUMS(bl.xb), TL(bl.xa), TL(bl.xb), bl.Win};
  // h = conv0(resample(silu(norm0(x))))
  const int rs = b.up ? RS_UP : (b.down ? RS_DOWN : RS_NONE);
  ConvArgs c0 = conv(b.conv0, xa, Ca, xb, Cb, bl.Hin, bl.Win, bl.H, bl.W, bl.h, st);
  c0.coef = CF(bl.coef0); c0.coef_batch = 1; c0.act = 1; c0.resample = rs;
  if ((rc = gn_for_conv(g0, c0, /*need_table=*/bl.xd >= 0, s))) return rc;
  if (bl.xd >= 0) {
    WgradArgs m{};
    m.xa = xa; m.xb = xb; m.Ca = Ca; m.Cb = Cb; m.coef = c0.coef; m.coef_batch = 1; m.act = 1; m.resample = RS_DOWN;
    m.Hs = bl.Hin; m.Ws = bl.Win; m.H = bl.H; m.W = bl.W; m.B = B;
    if ((rc = launch_act_materialize(m, T(bl.xd), s))) return rc;
    c0.xa = T(bl.xd); c0.xb = nullptr; c0.Ca = Ca + Cb; c0.Cb = 0;
    c0.coef = nullptr; c0.act = 0; c0.resample = RS_NONE; c0.Hs = bl.H; c0.Ws = bl.W;
  }
  if ((rc = launch_conv(c0, 9, s))) return rc;
  // norm1 + FiLM -> transform table for conv1
  GnArgs g1{T(bl.h), nullptr, b.cout, 0, bl.H * bl.W, B, b.norm1.groups, pk + b.norm1.gamma, pk + b.norm1.beta,
            film() + b.film_row0, coef_batch(), P.film_rows, eps, CF(bl.coef1), T(bl.stats1), SUMS(bl.h), nullptr, TL(bl.h), SumTiles{}, bl.W};
  // skip path
  const float* res = xa;
  int res_mode = RS_NONE;
  const bool fold_skip = b.skip_kernel == 1 && (bl.sk < 0 || bl.wfold);      // see build_layout
  if (b.skip_kernel == 1 && !fold_skip) {
    ConvArgs cs = conv(b.skip, xa, Ca, xb, Cb, bl.Hin, bl.Win, bl.H, bl.W, bl.sk, st);
    cs.resample = rs;
    if ((rc = launch_conv(cs, 1, s))) return rc;
    res = T(bl.sk);
  } else if (b.skip_kernel == 0) {
    res_mode = rs;
  }
  // y = conv1(silu(film(norm1(h)))) + skip
  ConvArgs c1 = conv(b.conv1, T(bl.h), b.cout, nullptr, 0, bl.H, bl.W, bl.H, bl.W, bl.y, st);
  c1.coef = CF(bl.coef1); c1.coef_batch = 1; c1.act = 1;
  c1.res = res; c1.res_mode = res_mode;
  if (fold_skip) {            // y = conv1(...) + skip(orig): the projection rides on conv1 as extra K chunks
    c1.res = nullptr; c1.res_mode = RS_NONE;
    c1.sk_xa = xa; c1.sk_xb = xb; c1.sk_Ca = Ca; c1.sk_Cb = Cb;
    c1.sk_wpk = pk + b.skip.wpk; c1.sk_bias = pk + b.skip.bias;
    c1.sk_wfrag = b.skip.wfrag != NONE ? pk + b.skip.wfrag : nullptr;
  }
  if ((rc = gn_for_conv(g1, c1, /*need_table=*/bl.xd1 >= 0, s))) return rc;
  if (bl.xd1 >= 0) {          // dropout: xd1 = mask * s * silu(film(norm1(h))) by one pass, and conv1 on it as conv0 on a down block's xd
    if ((rc = launch_dropout_act(T(bl.h), c1.coef, 1, T(bl.xd1), B, b.cout, bl.H, bl.W, P.dropout_p, seed_slot(),
                                 (unsigned long long)bl.draw, s))) return rc;
    c1.xa = T(bl.xd1); c1.coef = nullptr; c1.act = 0;
  }
  if ((rc = launch_conv(c1, 9, s))) return rc;
  if (!b.attn) return MCEDM_OK;
  // attention: z = proj(attn(qkv(norm2(y)))) + y
  if (bl.stats2 < 0 && attn_block_fused_applicable(b.cout, b.heads, bl.H, bl.W, b.norm2.groups))     // inference, 8 x 8 x 64: one launch
    return launch_attn_block64(T(bl.y), T(bl.z), pk + b.norm2.gamma, pk + b.norm2.beta, eps, b.norm2.groups, pk + b.qkv.wpk,
                               pk + b.qkv.bias, pk + b.proj.wpk, pk + b.proj.bias, SUMS(bl.z), &st[bl.z], B, s);
  GnArgs g2{T(bl.y), nullptr, b.cout, 0, bl.H * bl.W, B, b.norm2.groups, pk + b.norm2.gamma, pk + b.norm2.beta,
            nullptr, 0, 0, eps, CF(bl.coef2), T(bl.stats2), SUMS(bl.y), nullptr, TL(bl.y), SumTiles{}, bl.W};
  ConvArgs cq = conv(b.qkv, T(bl.y), b.cout, nullptr, 0, bl.H, bl.W, bl.H, bl.W, bl.qkv, st);
  cq.coef = CF(bl.coef2); cq.coef_batch = 1; cq.act = 0;
  if ((rc = gn_for_conv(g2, cq, false, s))) return rc;
  if ((rc = launch_conv(cq, 1, s))) return rc;
  if ((rc = launch_attention(T(bl.qkv), T(bl.a), B, b.heads, bl.H * bl.W, s))) return rc;
  ConvArgs cp = conv(b.proj, T(bl.a), b.cout, nullptr, 0, bl.H, bl.W, bl.H, bl.W, bl.z, st);
  cp.res = T(bl.y); cp.res_mode = RS_NONE;
  return launch_conv(cp, 1, s);
}

// ---- dx_cond head (adm_blocks.py:334-362) ------------------------------------------------------------------
// out[B, cx + cd, HW] = cat(x[B, cx, HW], dx[B, cd, HW] or zeros)   (cat_dx: adm_blocks.py:335-339)
__global__ void concat_x_dx_kernel(const float* __restrict__ x, const float* __restrict__ dx, int cx, int cd, size_t hw,
                                   size_t total, float* __restrict__ out) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const size_t per = (size_t)(cx + cd) * hw;
    const size_t n = i / per, r = i - n * per;
    out[i] = r < (size_t)cx * hw ? x[n * cx * hw + r] : (dx ? dx[n * cd * hw + (r - (size_t)cx * hw)] : 0.f);
  }
}
// torch.nn.GELU() (approximate='none'): y = 0.5 v (1 + erf(v / sqrt(2)));  mode 1: out = g * dGELU(v)
__global__ void gelu_kernel(const float* __restrict__ v, const float* g, float* out, size_t n, int mode) {      // out may be g
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const float a = v[i];
    const float cdf = 0.5f * (1.0f + erff(a * 0.70710678118654752440f));
    out[i] = mode ? g[i] * (cdf + a * 0.39894228040143267794f * expf(-0.5f * a * a)) : a * cdf;
  }
}
int launch_gelu(const float* v, const float* g, float* out, size_t n, int mode, hipStream_t s) {
  const size_t b = (n + 255) / 256;
  hipLaunchKernelGGL(gelu_kernel, dim3((unsigned)(b < 4096 ? (b ? b : 1) : 4096)), dim3(256), 0, s, v, g, out, n, mode);
  MCEDM_LAUNCH_CHECK("gelu_kernel");
  return MCEDM_OK;
}

int AdmNet::forward(const AdmIn& in, float* out) const {
  const mcedm_plan& P = *plan;
  const int ch = P.desc.ch;
  const int dxm = P.desc.dx_mode;
  int rc;
  EmbArgs e{in.noise_labels, n_noise, ch, pk + P.freqs, pk + P.w0, pk + P.b0, pk + P.w1, pk + P.b1,
            pk + P.waff, pk + P.baff, P.film_rows, nullptr, T(L.film)};
  if ((rc = launch_embedding(e, s))) return rc;
  // dropout: the seed of this pass goes into the workspace, on the stream; this pass's kernels and the backward's read it there
  if (dropout())
    MCEDM_HIP_TRY(hipMemcpyAsync(act + L.t[L.seed].off, P.dropout_seed, sizeof(unsigned long long), hipMemcpyDeviceToDevice, s));
  std::vector<SumTiles> st(L.t.size());     // tiling of each tensor's fused-statistics table
  // conv_in on cat(cond, x)  (cond FIRST, adm_blocks.py:332)
  const float* xb = in.x;
  int Cb = P.desc.in_channels;
  if (dxm == MCEDM_DX_CAT) {         // cat(cond, x, dx): x and dx meet in one staging tensor (the kernels take two sources)
    const size_t hw = (size_t)H * W, total = (size_t)B * (P.desc.in_channels + P.desc.dx_channels) * hw;
    const size_t nb = (total + 255) / 256;
    hipLaunchKernelGGL(concat_x_dx_kernel, dim3((unsigned)(nb < 4096 ? nb : 4096)), dim3(256), 0, s, in.x, in.dx, P.desc.in_channels,
                       P.desc.dx_channels, hw, total, T(L.xdx));
    MCEDM_LAUNCH_CHECK("concat_x_dx_kernel");
    xb = T(L.xdx); Cb = P.desc.in_channels + P.desc.dx_channels;
  }
  // (conv_in and out_conv never take the Winograd kernel, whatever their channel counts)
  ConvArgs ci = conv(P.conv_in, in.cond, P.desc.cond_channels, xb, Cb, H, W, H, W, dxm == MCEDM_DX_ENC ? L.xf : L.t0, st);
  ci.wino = nullptr;
  ci.coef = in.coef_in; ci.coef_batch = coef_batch(); ci.act = 0;
  if ((rc = launch_conv(ci, 9, s))) return rc;
  if (dxm == MCEDM_DX_ENC) {
    // x_feat = combine_enc(cat(conv_in(.), dx_enc(dx))), dx_enc = Conv3x3 -> GELU -> Conv3x3; dx None: zero features, NOT
    // dx_enc(0) (adm_blocks.py:352-362)
    const int c0 = P.conv_in.cout;
    if (in.dx) {
      ConvArgs ca = conv(P.dx_enc0, in.dx, P.desc.dx_channels, nullptr, 0, H, W, H, W, L.d1, st);
      if ((rc = launch_conv(ca, 9, s))) return rc;
      if ((rc = launch_gelu(T(L.d1), nullptr, T(L.g1), (size_t)B * c0 * H * W, 0, s))) return rc;
      ConvArgs cb = conv(P.dx_enc2, T(L.g1), c0, nullptr, 0, H, W, H, W, L.d2, st);
      if ((rc = launch_conv(cb, 9, s))) return rc;
    } else {
      MCEDM_HIP_TRY(hipMemsetAsync(T(L.d2), 0, L.t[L.d2].bytes, s));
    }
    ConvArgs cc = conv(P.combine, T(L.xf), c0, T(L.d2), c0, H, W, H, W, L.t0, st);
    if ((rc = launch_conv(cc, 9, s))) return rc;
  }
  size_t bi = 0;
  for (const BlockP& b : P.enc) if ((rc = run_block(b, L.blocks[bi++], st))) return rc;
  for (const BlockP& b : P.dec) if ((rc = run_block(b, L.blocks[bi++], st))) return rc;
  // out = out_conv(silu(out_norm(x)))
  const TRef& last = L.t[L.last];
  GnArgs go{T(L.last), nullptr, last.C, 0, H * W, B, P.out_norm.groups, pk + P.out_norm.gamma,
            pk + P.out_norm.beta, nullptr, 0, 0, 1e-5f, CF(L.coef_out), T(L.stats_out), SUMS(L.last), nullptr, st[L.last],
            SumTiles{}, W};
  ConvArgs co = conv(P.conv_out, T(L.last), last.C, nullptr, 0, H, W, H, W, -1, st);
  co.wino = nullptr;
  co.out = out;
  co.coef = CF(L.coef_out); co.coef_batch = 1; co.act = 1;
  if ((rc = gn_for_conv(go, co, false, s))) return rc;
  return launch_conv(co, 9, s);
}

__global__ void scale_to_coef_kernel(const float* __restrict__ x_scale, int n, int cond_ch, int in_ch, int dx_ch, Coef* out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int Ct = cond_ch + in_ch + dx_ch;
  for (int c = 0; c < Ct; ++c) out[(size_t)i * Ct + c] = Coef{0.f, (c < cond_ch || c >= cond_ch + in_ch) ? 1.0f : x_scale[i], 0.f, 0.f};
}

int denoise_impl(const AdmNet& net, const float* x, const float* dx, const float* cond, const float* sigma_dev, float sigma_host,
                 double w, float sigma_data, float* D_out, float* F_out) {
  const mcedm_unet_desc& d = net.plan->desc;
  int rc;
  if ((rc = launch_precond_prepare(sigma_dev, sigma_host, sigma_dev ? 0 : 1, net.n_noise, sigma_data, d.cond_channels, d.in_channels,
                                   d.dx_mode == MCEDM_DX_CAT ? d.dx_channels : 0, net.coefs4(), net.c_noise(), net.coef_in(),
                                   net.s))) return rc;
  // classifier-free branch, mcedm.py:453-458; models/ddim.py:1755-1760: taken when cond OR dx is given, and the
  // unconditional evaluation drops both
  float* Fu = std::fabs(w) >= 0.001 && (cond != nullptr || dx != nullptr) ? net.Fu() : nullptr;
  if ((rc = net.forward_cfg(AdmIn{x, dx, cond, net.coef_in(), net.c_noise()}, net.F(), Fu))) return rc;
  const size_t per = (size_t)d.out_channels * net.H * net.W;
  return launch_precond_finish(x, net.F(), Fu, w, net.coefs4(), net.n_noise, per, per * net.B, D_out, F_out, net.s);
}

}  // namespace mcedm

extern "C" int mcedm_unet_workspace_bytes(const mcedm_plan* plan, int B, int H, int W, int training, size_t* bytes) {
  VariantScope variant_scope__(plan);
  MCEDM_REQUIRE(plan && bytes, "workspace_bytes: null argument");
  AdmNet net;
  const int rc = adm_sizes(*plan, B, H, W, training, B, &net, bytes);
  if (rc == MCEDM_OK && training) *bytes += backward_scratch_bytes(*plan, net.L, B, H, W);
  return rc;
}

extern "C" int mcedm_unet_forward_dx(const mcedm_plan* plan, const void* packed, const float* x, const float* dx, const float* cond,
                                     const float* x_scale, const float* noise_labels, int n_noise, float* out,
                                     void* workspace, size_t workspace_bytes, int B, int H, int W, int training,
                                     void* stream) {
  VariantScope variant_scope__(plan);
  MCEDM_REQUIRE(plan && packed && x && noise_labels && out && workspace, "unet_forward: null argument");
  MCEDM_REQUIRE(dx == nullptr || plan->desc.dx_mode != MCEDM_DX_NONE, "unet_forward: dx given to a plan without dx_cond");
  AdmNet net;
  const int rc = adm_bind("unet_forward", *plan, packed, workspace, workspace_bytes, 0, no_extra, B, H, W, training, n_noise, stream, &net);
  if (rc) return rc;
  AdmIn in{x, dx, cond, nullptr, noise_labels};
  if (x_scale) {
    hipLaunchKernelGGL(scale_to_coef_kernel, dim3(ceil_div(n_noise, 64)), dim3(64), 0, net.s, x_scale, n_noise,
                       plan->desc.cond_channels, plan->desc.in_channels,
                       plan->desc.dx_mode == MCEDM_DX_CAT ? plan->desc.dx_channels : 0, net.coef_in());
    MCEDM_LAUNCH_CHECK("scale_to_coef_kernel");
    in.coef_in = net.coef_in();
  }
  return net.forward(in, out);
}

extern "C" int mcedm_unet_forward(const mcedm_plan* plan, const void* packed, const float* x, const float* cond,
                                  const float* x_scale, const float* noise_labels, int n_noise, float* out,
                                  void* workspace, size_t workspace_bytes, int B, int H, int W, int training,
                                  void* stream) {
  VariantScope variant_scope__(plan);
  return mcedm_unet_forward_dx(plan, packed, x, nullptr, cond, x_scale, noise_labels, n_noise, out, workspace, workspace_bytes, B, H,
                               W, training, stream);
}

extern "C" int mcedm_edm_denoise_dx(const mcedm_plan* plan, const void* packed, const float* x, const float* dx, const float* sigma,
                                    int n_sigma, const float* cond, float* D_out, float* F_out, void* workspace,
                                    size_t workspace_bytes, int B, int H, int W, int training, double sigma_data,
                                    void* stream) {
  VariantScope variant_scope__(plan);
  MCEDM_REQUIRE(plan && packed && x && sigma && D_out && workspace, "edm_denoise: null argument");
  MCEDM_REQUIRE(dx == nullptr || plan->desc.dx_mode != MCEDM_DX_NONE, "edm_denoise: dx given to a plan without dx_cond");
  AdmNet net;
  const int rc = adm_bind("edm_denoise", *plan, packed, workspace, workspace_bytes, 0, no_extra, B, H, W, training, n_sigma, stream, &net);
  return rc ? rc : denoise_impl(net, x, dx, cond, sigma, 0.f, 0.0, (float)sigma_data, D_out, F_out);
}

extern "C" int mcedm_edm_denoise(const mcedm_plan* plan, const void* packed, const float* x, const float* sigma,
                                 int n_sigma, const float* cond, float* D_out, float* F_out, void* workspace,
                                 size_t workspace_bytes, int B, int H, int W, int training, double sigma_data,
                                 void* stream) {
  VariantScope variant_scope__(plan);
  return mcedm_edm_denoise_dx(plan, packed, x, nullptr, sigma, n_sigma, cond, D_out, F_out, workspace, workspace_bytes, B, H, W,
                              training, sigma_data, stream);
}
