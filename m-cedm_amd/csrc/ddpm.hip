// ddpm.hip -- SURVEY.md section 8 f1: the DDPM U-Net (models/ddim_blocks.py:222-470) and the RePaint-style EDM sampler
// of PlDdim (models/ddim.py:915-1051) on the kernels of this library.
//
// The network is the ermongroup/ddim U-Net: ResnetBlock = GroupNorm(32, eps 1e-6) -> swish -> conv3x3 -> + temb_proj(swish(temb))
// -> GroupNorm -> swish -> conv3x3 -> + (1x1 nin_shortcut(x) | x); AttnBlock = GroupNorm -> q, k, v 1x1 -> one head over
// all C channels -> proj_out + x; Downsample = pad (0,1,0,1) + conv3x3 stride 2; Upsample = nearest 2x + conv3x3.
// Mapping onto the existing kernels:
//   * GroupNorm + swish are the per-(sample, channel) transform rows a conv applies while staging its input (fused from the
//     producer's epilogue statistics when the 32 groups are whole 4-channel blocks, else one gn_coef_kernel pass);
//   * the timestep term temb_proj(swish(temb)) is constant over the batch while sampling (one sigma per call), so it is
//     folded into conv1's bias vector by ddpm_temb_kernel: no extra pass, and the fused statistics see it;
//   * q, k, v are one packed [3C x C] GEMM whose output is the attention kernel's [3][64][T] layout (C == 64);
//   * the stride-2 conv is conv_s2_mfma_kernel (4-phase LDS tile), nearest-up is the RS_UP staging mode, the channel
//     concat of the decoder is virtual (two source pointers).
// Only the forward is built.  The samplers evaluate it at one timestep per call; the noising pass of training at one per sample
// (the last section of this file): there the table of bias rows holds a row set per sample and conv1 reads its sample's.
//   * the conditioning head of the single-task model (cond_enc / combine_enc, ddim_blocks.py:279-306, 401-421) is folded into
//     conv_in at pack time (combine_enc is linear); what depends on cond is one map M [B, ch, R, R], computed by
//     ddpm_cond_map_kernel once per sampler call and added by conv_in as its residual, in front of the fused statistics.
//   * cat_cond (ddim_blocks.py:259, 386-391; configs/model/edm_cond_h_res32.yaml): conv_in reads cat(cond, x) through its two
//     source pointers, cond first; a null cond source reads as zeros (cond None).  No head, no map, no extra launch.
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "heun.hpp"
#include "prof.hpp"

namespace mcedm {

struct DConv { int w = -1, b = -1; int cin = 0, cout = 0, taps = 0; size_t wpk = NONE, bias = NONE, wino = NONE; };   // wino: Winograd table (conv_wino.hip)
struct DNorm { int w = -1, b = -1; int C = 0; size_t gamma = NONE, beta = NONE; };
struct DRes {
  std::string key;
  int cin = 0, cout = 0;
  DNorm n1, n2;
  DConv c1, c2, sc;
  bool has_sc = false;
  int tw = -1, tb = -1;      // temb_proj parameters
  int brow = 0;              // first row of this block in the combined (conv1.bias + temb_proj) bias table
};
struct DAttn {
  std::string key;
  int C = 0;
  DNorm n;
  int qw[3] = {-1, -1, -1}, qb[3] = {-1, -1, -1};
  DConv qkv, proj;           // qkv.w / qkv.b unused: packed from the three parameters through qkv_src
  size_t qkv_src = NONE;     // scratch inside the packed buffer: [3C][C] concatenated q, k, v weights
};
struct DLevel {
  std::vector<DRes> blocks;
  std::vector<DAttn> attns;
  bool has_rs = false;
  DConv rs;                  // downsample / upsample conv
};

}  // namespace mcedm

struct mcedm_ddpm_plan {
  mcedm_ddpm_desc desc;
  std::vector<mcedm::ParamInfo> params;
  int d0w = -1, d0b = -1, d1w = -1, d1b = -1;
  mcedm::DConv conv_in, conv_out;
  mcedm::DNorm norm_out;
  std::vector<mcedm::DLevel> down, up;
  mcedm::DRes mid1, mid2;
  mcedm::DAttn mid_attn;
  mcedm::KernelVariants variants;   // per-plan kernel choices (mcedm_ddpm_plan_set_variant); -1 = process default
  int rows = 0;              // total rows of the combined bias table (sum of cout over the ResnetBlocks)
  // packed buffer (float offsets)
  size_t freqs = mcedm::NONE, w0 = mcedm::NONE, b0 = mcedm::NONE, w1 = mcedm::NONE, b1 = mcedm::NONE;
  size_t tproj_w = mcedm::NONE, tproj_b = mcedm::NONE, c1bias = mcedm::NONE;
  size_t packed_floats = 0;
  int in_total = 0;          // conv_in input channels (self-conditioning or cat_cond channels first)
  int cat_channels = 0;      // cat_cond: the conditioning channels conv_in reads in front of the state (no head then)
  // the cond_enc / combine_enc head (mcedm_ddpm_plan_create_cond; cond_channels 0 = none).  Packed: cond_enc.0 as it is, the
  // folded 3x3 of the map as [tap][cin][cout], the map's bias, and the folded conv_in weight in parameter layout (the
  // source launch_pack_conv reads; conv_in.wpk / conv_in.bias hold the folded forms, the bias that of cond = None)
  int cond_channels = 0;
  int e0w = -1, e0b = -1, e2w = -1, e2b = -1, cbw = -1, cbb = -1;
  size_t enc0_w = mcedm::NONE, enc0_b = mcedm::NONE, map_w = mcedm::NONE, map_b = mcedm::NONE, in_fold = mcedm::NONE;
};

namespace mcedm {

static DNorm dnorm(mcedm_ddpm_plan& P, const std::string& k, int C) {
  DNorm n; n.C = C;
  n.w = add_param(P.params, k + ".weight", {C}); n.b = add_param(P.params, k + ".bias", {C});
  return n;
}
static DConv dconv(mcedm_ddpm_plan& P, const std::string& k, int cin, int cout, int ks) {
  DConv c; c.cin = cin; c.cout = cout; c.taps = ks * ks;
  c.w = add_param(P.params, k + ".weight", {cout, cin, ks, ks}); c.b = add_param(P.params, k + ".bias", {cout});
  return c;
}
// registration order of ResnetBlock.__init__ (ddim_blocks.py:116-142)
static DRes dres(mcedm_ddpm_plan& P, const std::string& k, int cin, int cout) {
  const int temb = 4 * P.desc.ch;
  DRes r; r.key = k; r.cin = cin; r.cout = cout;
  r.n1 = dnorm(P, k + ".norm1", cin);
  r.c1 = dconv(P, k + ".conv1", cin, cout, 3);
  r.tw = add_param(P.params, k + ".temb_proj.weight", {cout, temb}); r.tb = add_param(P.params, k + ".temb_proj.bias", {cout});
  r.n2 = dnorm(P, k + ".norm2", cout);
  r.c2 = dconv(P, k + ".conv2", cout, cout, 3);
  if (cin != cout) { r.has_sc = true; r.sc = dconv(P, k + ".nin_shortcut", cin, cout, 1); }
  r.brow = P.rows; P.rows += cout;
  return r;
}
// AttnBlock.__init__ (ddim_blocks.py:168-192)
static DAttn dattn(mcedm_ddpm_plan& P, const std::string& k, int C) {
  DAttn a; a.key = k; a.C = C;
  a.n = dnorm(P, k + ".norm", C);
  const char* names[3] = {"q", "k", "v"};
  for (int i = 0; i < 3; ++i) {
    a.qw[i] = add_param(P.params, k + "." + names[i] + ".weight", {C, C, 1, 1});
    a.qb[i] = add_param(P.params, k + "." + names[i] + ".bias", {C});
  }
  a.qkv.cin = C; a.qkv.cout = 3 * C; a.qkv.taps = 1;
  a.proj = dconv(P, k + ".proj_out", C, C, 1);
  return a;
}
static void dplace(Taker& t, DConv& c) {
  c.wpk = t.take(conv_packed_floats(c.cout, c.cin, c.taps));
  c.bias = t.take((size_t)(c.cout + 31) / 32 * 32);
  if (c.taps == 9 && c.cout % 64 == 0 && c.cin % 8 == 0) c.wino = t.take(conv_wino_packed_floats(c.cout, c.cin));
}
static void dplace(Taker& t, DNorm& n) { n.gamma = t.take(n.C); n.beta = t.take(n.C); }
static void dplace(Taker& t, DRes& r) {
  dplace(t, r.n1); dplace(t, r.c1); dplace(t, r.n2); dplace(t, r.c2);
  if (r.has_sc) dplace(t, r.sc);
}
static void dplace(Taker& t, DAttn& a) {
  dplace(t, a.n); dplace(t, a.qkv); dplace(t, a.proj);
  a.qkv_src = t.take((size_t)3 * a.C * a.C);
}

}  // namespace mcedm

using namespace mcedm;

// cond_channels: of the cond_enc head; cat_channels: of a cat_cond input (at most one of the two is non-zero)
static int ddpm_plan_build(const mcedm_ddpm_desc* d, int cond_channels, int cat_channels, mcedm_ddpm_plan** out) {
  MCEDM_REQUIRE(d && out, "ddpm_plan_create: null argument");
  MCEDM_REQUIRE(d->n_levels >= 1 && d->n_levels <= MCEDM_MAX_LEVELS, "ddpm_plan_create: n_levels=%d out of range", d->n_levels);
  MCEDM_REQUIRE(d->n_attn_resolutions >= 0 && d->n_attn_resolutions <= MCEDM_MAX_LEVELS, "ddpm_plan_create: bad n_attn_resolutions");
  MCEDM_REQUIRE(d->in_channels > 0 && d->out_channels > 0 && d->num_res_blocks >= 1, "ddpm_plan_create: bad channel / block counts");
  MCEDM_REQUIRE(d->ch >= 32 && d->ch % 32 == 0, "ddpm_plan_create: ch=%d must be a multiple of 32 (GroupNorm(32), ddim_blocks.py:62)", d->ch);
  MCEDM_REQUIRE(d->resolution > 0 && d->resolution % (1 << (d->n_levels - 1)) == 0, "ddpm_plan_create: resolution %d not divisible by 2^(levels-1)", d->resolution);
  for (int l = 0; l < d->n_levels; ++l) MCEDM_REQUIRE(d->ch_mult[l] >= 1, "ddpm_plan_create: ch_mult[%d] < 1", l);
  mcedm_ddpm_plan* Pp = new mcedm_ddpm_plan();
  mcedm_ddpm_plan& P = *Pp;
  P.desc = *d;
  const int ch = d->ch, temb = 4 * ch, L = d->n_levels;
  P.cat_channels = cat_channels;
  P.in_total = cat_channels + d->in_channels * (d->self_cond ? 2 : 1);      // cat(cond, cat(x_self_cond, x)), ddim_blocks.py:258-259
  // registration order of Model.__init__ (ddim_blocks.py:252-362)
  P.d0w = add_param(P.params, "temb.dense.0.weight", {temb, ch}); P.d0b = add_param(P.params, "temb.dense.0.bias", {temb});
  P.d1w = add_param(P.params, "temb.dense.1.weight", {temb, temb}); P.d1b = add_param(P.params, "temb.dense.1.bias", {temb});
  P.conv_in = dconv(P, "conv_in", P.in_total, ch, 3);
  P.cond_channels = cond_channels;
  if (cond_channels > 0) {             // cond_enc = Sequential(Conv1x1, GELU, Conv3x3 circular), combine_enc (ddim_blocks.py:281-304)
    P.e0w = add_param(P.params, "cond_enc.0.weight", {ch, cond_channels, 1, 1}); P.e0b = add_param(P.params, "cond_enc.0.bias", {ch});
    P.e2w = add_param(P.params, "cond_enc.2.weight", {ch, ch, 3, 3}); P.e2b = add_param(P.params, "cond_enc.2.bias", {ch});
    P.cbw = add_param(P.params, "combine_enc.weight", {ch, 2 * ch, 1, 1}); P.cbb = add_param(P.params, "combine_enc.bias", {ch});
  }
  int res = d->resolution, block_in = ch;
  auto in_mult = [&](int l) { return l == 0 ? 1 : d->ch_mult[l - 1]; };
  P.down.resize(L);
  for (int l = 0; l < L; ++l) {
    DLevel& lv = P.down[l];
    const std::string k = "down." + std::to_string(l);
    block_in = ch * in_mult(l);
    const int block_out = ch * d->ch_mult[l];
    for (int j = 0; j < d->num_res_blocks; ++j) {
      lv.blocks.push_back(dres(P, k + ".block." + std::to_string(j), block_in, block_out));
      block_in = block_out;
    }
    if (in_list(d->attn_resolutions, d->n_attn_resolutions, res))
      for (int j = 0; j < d->num_res_blocks; ++j) lv.attns.push_back(dattn(P, k + ".attn." + std::to_string(j), block_in));
    if (l != L - 1) { lv.has_rs = true; lv.rs = dconv(P, k + ".downsample.conv", block_in, block_in, 3); res /= 2; }
  }
  P.mid1 = dres(P, "mid.block_1", block_in, block_in);
  P.mid_attn = dattn(P, "mid.attn_1", block_in);
  P.mid2 = dres(P, "mid.block_2", block_in, block_in);
  // the up path is BUILT from the deepest level (block_in chains that way) but REGISTERED level 0 first
  // (`self.up.insert(0, up)`, ddim_blocks.py:351): build into a temporary parameter list per level, then append in order
  P.up.resize(L);
  std::vector<std::vector<ParamInfo>> up_params(L);
  std::vector<ParamInfo> saved = P.params;
  for (int l = L - 1; l >= 0; --l) {
    P.params.clear();
    DLevel& lv = P.up[l];
    const std::string k = "up." + std::to_string(l);
    const int block_out = ch * d->ch_mult[l];
    int skip_in = ch * d->ch_mult[l];
    for (int j = 0; j < d->num_res_blocks + 1; ++j) {
      if (j == d->num_res_blocks) skip_in = ch * in_mult(l);
      lv.blocks.push_back(dres(P, k + ".block." + std::to_string(j), block_in + skip_in, block_out));
      block_in = block_out;
    }
    if (in_list(d->attn_resolutions, d->n_attn_resolutions, res))
      for (int j = 0; j < d->num_res_blocks + 1; ++j) lv.attns.push_back(dattn(P, k + ".attn." + std::to_string(j), block_in));
    if (l != 0) { lv.has_rs = true; lv.rs = dconv(P, k + ".upsample.conv", block_in, block_in, 3); res *= 2; }
    up_params[l] = P.params;
  }
  // re-number: parameter indices inside level l are local to up_params[l]; shift them to their final position
  P.params = saved;
  auto shift_conv = [](DConv& c, int by) { if (c.w >= 0) { c.w += by; c.b += by; } };
  auto shift_norm = [](DNorm& n, int by) { n.w += by; n.b += by; };
  for (int l = 0; l < L; ++l) {
    const int by = (int)P.params.size();
    DLevel& lv = P.up[l];
    for (DRes& r : lv.blocks) {
      shift_norm(r.n1, by); shift_conv(r.c1, by); r.tw += by; r.tb += by; shift_norm(r.n2, by); shift_conv(r.c2, by);
      if (r.has_sc) shift_conv(r.sc, by);
    }
    for (DAttn& a : lv.attns) {
      shift_norm(a.n, by);
      for (int i = 0; i < 3; ++i) { a.qw[i] += by; a.qb[i] += by; }
      shift_conv(a.proj, by);
    }
    if (lv.has_rs) shift_conv(lv.rs, by);
    P.params.insert(P.params.end(), up_params[l].begin(), up_params[l].end());
  }
  P.norm_out = dnorm(P, "norm_out", block_in);
  P.conv_out = dconv(P, "conv_out", block_in, d->out_channels, 3);
  // the rows of the combined bias table in the order of the parameter table's temb_proj entries (mcedm_ddpm_temb_rows hands the
  // table out); dres numbered the up path in the order it was built, deepest level first
  {
    int row = 0;
    auto number = [&](DRes& r) { r.brow = row; row += r.cout; };
    for (DLevel& lv : P.down) for (DRes& r : lv.blocks) number(r);
    number(P.mid1); number(P.mid2);
    for (DLevel& lv : P.up) for (DRes& r : lv.blocks) number(r);
  }

  // every width that meets GroupNorm(32) must be a multiple of 32; attention is one head over all C channels and the
  // attention kernel is built for 64
  std::string bad;
  auto chk_res = [&](const DRes& r) { if (r.cin % 32 || r.cout % 32) bad = r.key; };
  auto chk_attn = [&](const DAttn& a) { if (a.C != 64) bad = a.key + " (attention over " + std::to_string(a.C) + " channels; only 64 is built)"; };
  for (auto* v : {&P.down, &P.up}) for (DLevel& lv : *v) { for (DRes& r : lv.blocks) chk_res(r); for (DAttn& a : lv.attns) chk_attn(a); }
  chk_res(P.mid1); chk_res(P.mid2); chk_attn(P.mid_attn);
  if (!bad.empty()) {
    set_error("ddpm_plan_create: unsupported block %s", bad.c_str());
    delete Pp;
    return MCEDM_ERR_UNSUPPORTED;
  }

  Taker t;
  P.freqs = t.take(ch / 2);
  P.w0 = t.take((size_t)temb * ch); P.b0 = t.take(temb);
  P.w1 = t.take((size_t)temb * temb); P.b1 = t.take(temb);
  P.tproj_w = t.take((size_t)P.rows * temb); P.tproj_b = t.take(P.rows); P.c1bias = t.take(P.rows);
  dplace(t, P.conv_in);
  for (auto* v : {&P.down, &P.up})
    for (DLevel& lv : *v) {
      for (DRes& r : lv.blocks) dplace(t, r);
      for (DAttn& a : lv.attns) dplace(t, a);
      if (lv.has_rs) dplace(t, lv.rs);
    }
  dplace(t, P.mid1); dplace(t, P.mid_attn); dplace(t, P.mid2);
  dplace(t, P.norm_out); dplace(t, P.conv_out);
  if (cond_channels > 0) {             // behind everything else: the offsets of a plan without the head do not move
    P.enc0_w = t.take((size_t)ch * cond_channels); P.enc0_b = t.take(ch);
    P.map_w = t.take((size_t)9 * ch * ch); P.map_b = t.take(ch);
    P.in_fold = t.take((size_t)ch * P.in_total * 9);
  }
  P.packed_floats = t.cur;
  *out = Pp;
  return MCEDM_OK;
}

extern "C" int mcedm_ddpm_plan_create(const mcedm_ddpm_desc* d, mcedm_ddpm_plan** out) { return ddpm_plan_build(d, 0, 0, out); }

extern "C" int mcedm_ddpm_plan_create_cond(const mcedm_ddpm_desc* d, const mcedm_ddpm_cond_desc* cd, mcedm_ddpm_plan** out) {
  MCEDM_REQUIRE(d && cd && out, "ddpm_plan_create_cond: null argument");
  MCEDM_REQUIRE(cd->cond_channels >= 0 && cd->cond_channels <= 64, "ddpm_plan_create_cond: cond_channels=%d outside [0, 64]", cd->cond_channels);
  const bool cat = cd->cat_cond && cd->cond_channels > 0;
  MCEDM_REQUIRE(!(cat && d->self_cond),
                "ddpm_plan_create_cond: cat_cond (the conditioning concatenated to the input of the DDPM U-Net, ddim_blocks.py:259, "
                "386-391) together with self_cond is not built; cat_cond needs self_cond 0");
  MCEDM_REQUIRE(!cat || cd->cond_channels + d->in_channels <= 64, "ddpm_plan_create_cond: cat_cond input of %d + %d channels (at most 64)",
                cd->cond_channels, d->in_channels);
  if (cat) return ddpm_plan_build(d, 0, cd->cond_channels, out);
  MCEDM_REQUIRE(cd->cond_channels == 0 || d->ch <= 512, "ddpm_plan_create_cond: ch=%d > 512 (the map kernel holds ch / 128 tiles per wave)", d->ch);
  return ddpm_plan_build(d, cd->cond_channels, 0, out);
}

extern "C" int mcedm_ddpm_plan_set_variant(mcedm_ddpm_plan* plan, int which, int value) {
  return plan_set_variant(plan, "ddpm_plan_set_variant", which, value);
}
extern "C" void mcedm_ddpm_plan_destroy(mcedm_ddpm_plan* plan) { delete plan; }
extern "C" int mcedm_ddpm_param_count(const mcedm_ddpm_plan* plan) { return plan_param_count(plan); }
extern "C" int mcedm_ddpm_param_info(const mcedm_ddpm_plan* plan, int index, const char** name, int64_t* numel, int32_t* ndim,
                                     int64_t shape[4]) {
  return plan_param_info(plan, "ddpm_param_info", index, name, numel, ndim, shape);
}
extern "C" int mcedm_ddpm_packed_bytes(const mcedm_ddpm_plan* plan, size_t* bytes) {
  return plan_packed_bytes(plan, "ddpm_packed_bytes", bytes);
}

// ------------------------------------------------------------------------------------------
// weight packing
// ------------------------------------------------------------------------------------------
namespace mcedm {

static int dcopy(float* dst, const float* src, size_t n, hipStream_t s) {
  MCEDM_HIP_TRY(hipMemcpyAsync(dst, src, n * sizeof(float), hipMemcpyDeviceToDevice, s));
  return MCEDM_OK;
}
static int dpack(const DConv& c, const float* const* params, float* pk, hipStream_t s) {
  int rc = launch_pack_conv(params[c.w], pk + c.wpk, c.cout, c.cin, c.taps, 0, 0, s);
  if (rc) return rc;
  if (c.wino != NONE && (rc = launch_pack_conv_wino(params[c.w], pk + c.wino, c.cout, c.cin, 0, s))) return rc;
  return dcopy(pk + c.bias, params[c.b], c.cout, s);
}
static int dpack(const DNorm& n, const float* const* params, float* pk, hipStream_t s) {
  int rc = dcopy(pk + n.gamma, params[n.w], n.C, s);
  if (rc) return rc;
  return dcopy(pk + n.beta, params[n.b], n.C, s);
}
static int dpack(const mcedm_ddpm_plan& P, const DRes& r, const float* const* params, float* pk, hipStream_t s) {
  const int temb = 4 * P.desc.ch;
  int rc;
  if ((rc = dpack(r.n1, params, pk, s)) || (rc = dpack(r.c1, params, pk, s)) || (rc = dpack(r.n2, params, pk, s)) ||
      (rc = dpack(r.c2, params, pk, s))) return rc;
  if (r.has_sc && (rc = dpack(r.sc, params, pk, s))) return rc;
  if ((rc = dcopy(pk + P.tproj_w + (size_t)r.brow * temb, params[r.tw], (size_t)r.cout * temb, s))) return rc;
  if ((rc = dcopy(pk + P.tproj_b + r.brow, params[r.tb], r.cout, s))) return rc;
  return dcopy(pk + P.c1bias + r.brow, params[r.c1.b], r.cout, s);
}
static int dpack(const DAttn& a, const float* const* params, float* pk, hipStream_t s) {
  int rc;
  if ((rc = dpack(a.n, params, pk, s))) return rc;
  const size_t cc = (size_t)a.C * a.C;
  for (int i = 0; i < 3; ++i) {       // rows [q; k; v]: with one head this IS the attention kernel's (which, c) order
    if ((rc = dcopy(pk + a.qkv_src + i * cc, params[a.qw[i]], cc, s))) return rc;
    if ((rc = dcopy(pk + a.qkv.bias + (size_t)i * a.C, params[a.qb[i]], a.C, s))) return rc;
  }
  if ((rc = launch_pack_conv(pk + a.qkv_src, pk + a.qkv.wpk, 3 * a.C, a.C, 1, 0, 0, s))) return rc;
  return dpack(a.proj, params, pk, s);
}


// The fold of the conditioning head, fp64 accumulation rounded once (Wx, Wc: the two halves of combine_enc.weight [ch][2 ch]):
//   [0, n0)        in_fold[o][i][tap] = sum_m Wx[o][m] conv_in.weight[m][i][tap]
//   [n0, n0 + n1)  map_w[tap][c][o]   = sum_m Wc[o][m] cond_enc.2.weight[m][c][tap]
//   then ch        bias[o]            = sum_m Wx[o][m] conv_in.bias[m] + combine_enc.bias[o]      (cond None: zero features, no b_enc2)
//                  map_b[o]           = that + sum_m Wc[o][m] cond_enc.2.bias[m]                  (what the map carries)
__global__ __launch_bounds__(256) void ddpm_fold_kernel(const float* __restrict__ comb, const float* __restrict__ comb_b,
                                                        const float* __restrict__ win, const float* __restrict__ bin,
                                                        const float* __restrict__ w2, const float* __restrict__ b2, int ch, int cin,
                                                        float* __restrict__ in_fold, float* __restrict__ map_w,
                                                        float* __restrict__ bias, float* __restrict__ map_b) {
  const size_t n0 = (size_t)ch * cin * 9, n1 = (size_t)9 * ch * ch, total = n0 + n1 + ch;
  for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
    double acc = 0.0;
    if (e < n0) {
      const int o = (int)(e / ((size_t)cin * 9)), r = (int)(e % ((size_t)cin * 9));
      for (int m = 0; m < ch; ++m) acc += (double)comb[(size_t)o * 2 * ch + m] * (double)win[(size_t)m * cin * 9 + r];
      in_fold[e] = (float)acc;
    } else if (e < n0 + n1) {
      const size_t f = e - n0;
      const int o = (int)(f % ch), c = (int)((f / ch) % ch), tap = (int)(f / ((size_t)ch * ch));
      for (int m = 0; m < ch; ++m) acc += (double)comb[(size_t)o * 2 * ch + ch + m] * (double)w2[((size_t)m * ch + c) * 9 + tap];
      map_w[f] = (float)acc;
    } else {
      const int o = (int)(e - n0 - n1);
      double accc = 0.0;
      for (int m = 0; m < ch; ++m) acc += (double)comb[(size_t)o * 2 * ch + m] * (double)bin[m];
      for (int m = 0; m < ch; ++m) accc += (double)comb[(size_t)o * 2 * ch + ch + m] * (double)b2[m];
      bias[o] = (float)(acc + (double)comb_b[o]);
      map_b[o] = (float)(acc + accc + (double)comb_b[o]);
    }
  }
}

// conv_in of a plan with the head: the folded weight and bias in conv_in's packed slots
static int dpack_head(const mcedm_ddpm_plan& P, const float* const* params, float* pk, hipStream_t s) {
  const int ch = P.desc.ch;
  const DConv& c = P.conv_in;
  const size_t total = (size_t)ch * P.in_total * 9 + (size_t)9 * ch * ch + ch;
  hipLaunchKernelGGL(ddpm_fold_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, params[P.cbw], params[P.cbb], params[c.w],
                     params[c.b], params[P.e2w], params[P.e2b], ch, P.in_total, pk + P.in_fold, pk + P.map_w, pk + c.bias, pk + P.map_b);
  MCEDM_LAUNCH_CHECK("ddpm_fold_kernel");
  int rc;
  if ((rc = launch_pack_conv(pk + P.in_fold, pk + c.wpk, c.cout, c.cin, c.taps, 0, 0, s))) return rc;
  if (c.wino != NONE && (rc = launch_pack_conv_wino(pk + P.in_fold, pk + c.wino, c.cout, c.cin, 0, s))) return rc;
  if ((rc = dcopy(pk + P.enc0_w, params[P.e0w], (size_t)ch * P.cond_channels, s))) return rc;
  return dcopy(pk + P.enc0_b, params[P.e0b], ch, s);
}

}  // namespace mcedm

extern "C" int mcedm_ddpm_pack_weights(const mcedm_ddpm_plan* plan, const float* const* params, const float* temb_freqs,
                                       void* packed, void* stream) {
  VariantScope variant_scope__(plan);
  MCEDM_REQUIRE(plan && params && temb_freqs && packed, "ddpm_pack_weights: null argument");
  const mcedm_ddpm_plan& P = *plan;
  for (size_t i = 0; i < P.params.size(); ++i)
    MCEDM_REQUIRE(params[i] != nullptr, "ddpm_pack_weights: parameter %zu (%s) is null", i, P.params[i].name.c_str());
  hipStream_t s = (hipStream_t)stream;
  float* pk = (float*)packed;
  const int ch = P.desc.ch, temb = 4 * ch;
  int rc;
  if ((rc = dcopy(pk + P.freqs, temb_freqs, ch / 2, s))) return rc;
  if ((rc = dcopy(pk + P.w0, params[P.d0w], (size_t)temb * ch, s)) || (rc = dcopy(pk + P.b0, params[P.d0b], temb, s)) ||
      (rc = dcopy(pk + P.w1, params[P.d1w], (size_t)temb * temb, s)) || (rc = dcopy(pk + P.b1, params[P.d1b], temb, s))) return rc;
  if ((rc = P.cond_channels > 0 ? dpack_head(P, params, pk, s) : dpack(P.conv_in, params, pk, s))) return rc;
  for (auto* v : {&P.down, &P.up})
    for (const DLevel& lv : *v) {
      for (const DRes& r : lv.blocks) if ((rc = dpack(P, r, params, pk, s))) return rc;
      for (const DAttn& a : lv.attns) if ((rc = dpack(a, params, pk, s))) return rc;
      if (lv.has_rs && (rc = dpack(lv.rs, params, pk, s))) return rc;
    }
  if ((rc = dpack(P, P.mid1, params, pk, s)) || (rc = dpack(P.mid_attn, params, pk, s)) || (rc = dpack(P, P.mid2, params, pk, s))) return rc;
  if ((rc = dpack(P.norm_out, params, pk, s))) return rc;
  return dpack(P.conv_out, params, pk, s);
}

// ------------------------------------------------------------------------------------------
// timestep embedding -> the combined bias rows of every ResnetBlock's conv1
// ------------------------------------------------------------------------------------------
namespace mcedm {

__device__ __forceinline__ float swish_d(float v) { return v * (1.0f / (1.0f + expf(-v))); }     // x * sigmoid(x), ddim_blocks.py:33-35

// get_timestep_embedding (ddim_blocks.py:12-30: [sin | cos] of t * freqs) -> dense0 -> swish -> dense1 (:413-416), then
// for every block row r: out[r] = temb_proj_r . swish(temb) + temb_proj.bias[r] + conv1.bias[r] (:149-151).
// grid = nsplit workgroups of 16 waves; each recomputes the small MLP (one wave per row, 16 rows in flight: the kernel is a
// chain of three dependent mat-vec products and runs once per U-Net evaluation) and writes its slice of the rows.
constexpr int TEMB_NT = 1024, TEMB_NW = TEMB_NT / 64;
// the rows of ONE timestep: workgroup blockIdx.x of gridDim.x writes its slice.  A row is one wave's sum in a fixed order, so its
// bits depend on (t, weights) alone: not on the split, and not on which of the two kernels below runs this body.
__device__ __forceinline__ void ddpm_temb_rows(float* sm, float t, int ch, const float* __restrict__ freqs,
                                               const float* __restrict__ w0, const float* __restrict__ b0,
                                               const float* __restrict__ w1, const float* __restrict__ b1,
                                               const float* __restrict__ wp, const float* __restrict__ bp,
                                               const float* __restrict__ c1b, int rows, float* __restrict__ out) {
  const int temb = 4 * ch, half = ch / 2;
  float* e0 = sm;              // [ch]
  float* e1 = sm + ch;         // [temb]
  float* e2 = e1 + temb;       // [temb]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int k = tid; k < ch; k += TEMB_NT) {
    const float arg = t * freqs[k < half ? k : k - half];
    e0[k] = (k < half) ? sinf(arg) : cosf(arg);
  }
  __syncthreads();
  for (int j = wave; j < temb; j += TEMB_NW) {
    float s = 0.f;
    for (int k = lane; k < ch; k += 64) s = fmaf(e0[k], w0[(size_t)j * ch + k], s);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    if (lane == 0) e1[j] = swish_d(s + b0[j]);
  }
  __syncthreads();
  for (int j = wave; j < temb; j += TEMB_NW) {
    float s = 0.f;
    for (int k = lane; k < temb; k += 64) s = fmaf(e1[k], w1[(size_t)j * temb + k], s);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    if (lane == 0) e2[j] = swish_d(s + b1[j]);          // every consumer applies swish to temb first
  }
  __syncthreads();
  const int per = (rows + gridDim.x - 1) / gridDim.x;
  const int r1 = min(rows, (int)(blockIdx.x + 1) * per);
  for (int r = blockIdx.x * per + wave; r < r1; r += TEMB_NW) {
    float s = 0.f;
    for (int k = lane; k < temb; k += 64) s = fmaf(e2[k], wp[(size_t)r * temb + k], s);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    if (lane == 0) out[r] = (s + bp[r]) + c1b[r];
  }
}
__global__ __launch_bounds__(TEMB_NT) void ddpm_temb_kernel(float t, int ch, const float* __restrict__ freqs,
                                                            const float* __restrict__ w0, const float* __restrict__ b0,
                                                            const float* __restrict__ w1, const float* __restrict__ b1,
                                                            const float* __restrict__ wp, const float* __restrict__ bp,
                                                            const float* __restrict__ c1b, int rows, float* __restrict__ out) {
  extern __shared__ float sm[];
  ddpm_temb_rows(sm, t, ch, freqs, w0, b0, w1, b1, wp, bp, c1b, rows, out);
}
// One timestep per sample (training draws them per sample, models/ddim.py:276-278): sample blockIdx.y reads t[blockIdx.y] from
// device memory -- no host read, so the launch can be captured -- and writes row set blockIdx.y of out [B][rows].
__global__ __launch_bounds__(TEMB_NT) void ddpm_temb_batch_kernel(const float* __restrict__ t, int ch, const float* __restrict__ freqs,
                                                                  const float* __restrict__ w0, const float* __restrict__ b0,
                                                                  const float* __restrict__ w1, const float* __restrict__ b1,
                                                                  const float* __restrict__ wp, const float* __restrict__ bp,
                                                                  const float* __restrict__ c1b, int rows, float* __restrict__ out) {
  extern __shared__ float sm[];
  ddpm_temb_rows(sm, t[blockIdx.y], ch, freqs, w0, b0, w1, b1, wp, bp, c1b, rows, out + (size_t)blockIdx.y * rows);
}

// rows_out [B][P.rows] <- the rows at t[b], both in device memory.  The rows are split over at most as many workgroups as the one-
// timestep launch uses, fewer when the batch already fills the device (a row's bits do not depend on the split).
static int launch_temb_rows(const mcedm_ddpm_plan& P, const float* pk, const float* t, int B, float* rows_out, hipStream_t s) {
  MCEDM_REQUIRE(B > 0 && B <= 65535, "ddpm_temb_rows: batch %d outside [1, 65535]", B);
  int nsplit = P.rows / 32; if (nsplit < 1) nsplit = 1; if (nsplit > 64) nsplit = 64;
  const int fill = ceil_div(512, B);
  if (nsplit > fill) nsplit = fill;
  const int ch = P.desc.ch, temb = 4 * ch;
  // per sample: every workgroup's copy of the MLP (ch x temb + temb x temb) and the rows once; the weights come from L2 after the first read
  ProfScope ps("ddpm_temb_batch_kernel", 2.0 * B * ((double)nsplit * temb * (ch + temb) + (double)P.rows * temb),
               4.0 * ((double)temb * (ch + temb) + (double)P.rows * (temb + B)), s);
  hipLaunchKernelGGL(ddpm_temb_batch_kernel, dim3(nsplit, B), dim3(TEMB_NT), (size_t)(ch + 8 * ch) * sizeof(float), s, t, ch, pk + P.freqs,
                     pk + P.w0, pk + P.b0, pk + P.w1, pk + P.b1, pk + P.tproj_w, pk + P.tproj_b, pk + P.c1bias, P.rows, rows_out);
  MCEDM_LAUNCH_CHECK("ddpm_temb_batch_kernel");
  return MCEDM_OK;
}

// ------------------------------------------------------------------------------------------
// the conditioning map M = (Wc cond_enc.2) (*)circ GELU(cond_enc.0(cond)) + bias   [B, ch, R, R]
// ------------------------------------------------------------------------------------------
// An implicit GEMM on the fp32 MFMA: output channels x pixels x (ch * 9).  A workgroup owns CM_PW pixels of one image row.
// Per chunk of CM_KC encoder channels it forms the GELU features of the three rows it reads (halo included) straight from
// cond while staging -- wrap-around on both axes, so the ch-channel feature tensor never exists -- then runs the nine
// taps out of LDS.  Wave w owns the 32-channel output tiles w, w + 4, ...; weights [tap][cin][cout] come from L2 (one
// coalesced 128-byte row per half-wave).  Runs once per sampler call: 1.2 GFLOP per sample at 128^2.
constexpr int CM_PW = 32, CM_KC = 64, CM_NT = 256, CM_TM = 4;
__global__ __launch_bounds__(CM_NT) void ddpm_cond_map_kernel(const float* __restrict__ cond, int cc, const float* __restrict__ w0,
                                                              const float* __restrict__ b0, const float* __restrict__ wm,
                                                              const float* __restrict__ bias, int ch, int R,
                                                              float* __restrict__ out) {
  __shared__ float g[CM_KC][3][CM_PW + 2];
  const int x0 = blockIdx.x * CM_PW, y = blockIdx.y, n = blockIdx.z;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 31, kh = lane >> 5;
  const int mtiles = ch / 32;
  f32x16 acc[CM_TM];
#pragma unroll
  for (int i = 0; i < CM_TM; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
  const size_t plane = (size_t)R * R;
  for (int c0 = 0; c0 < ch; c0 += CM_KC) {
    const int kc = min(CM_KC, ch - c0);                  // a multiple of 32
    __syncthreads();                                     // the previous chunk's readers are done
    for (int e = tid; e < kc * 3 * (CM_PW + 2); e += CM_NT) {
      const int c = e / (3 * (CM_PW + 2)), rem = e - c * (3 * (CM_PW + 2)), r = rem / (CM_PW + 2), cl = rem - r * (CM_PW + 2);
      const int yy = ((y + r - 1) % R + R) % R, xx = ((x0 + cl - 1) % R + R) % R;       // padding_mode='circular'
      float v = b0[c0 + c];
      for (int k = 0; k < cc; ++k) v = fmaf(w0[(size_t)(c0 + c) * cc + k], cond[((size_t)n * cc + k) * plane + (size_t)yy * R + xx], v);
      g[c][r][cl] = 0.5f * v * (1.0f + erff(v * 0.70710678118654752440f));              // nn.GELU(): the erf form
    }
    __syncthreads();
    for (int tap = 0; tap < 9; ++tap) {
      const int dy = tap / 3, dx = tap - 3 * dy;
      const float* wt = wm + ((size_t)tap * ch + c0) * ch;
      for (int k2 = 0; k2 < kc; k2 += 2) {
        const float b = g[k2 + kh][dy][col + dx];
#pragma unroll
        for (int i = 0; i < CM_TM; ++i) {
          const int mt = wave + i * (CM_NT / 64);
          if (mt < mtiles) acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(wt[(size_t)(k2 + kh) * ch + mt * 32 + col], b, acc[i], 0, 0, 0);
        }
      }
    }
  }
  const int x = x0 + col;
  if (x >= R) return;
#pragma unroll
  for (int i = 0; i < CM_TM; ++i) {
    const int mt = wave + i * (CM_NT / 64);
    if (mt >= mtiles) continue;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int o = mt * 32 + 4 * kh + (r & 3) + 8 * (r >> 2);
      out[((size_t)n * ch + o) * plane + (size_t)y * R + x] = acc[i][r] + bias[o];
    }
  }
}

static int launch_cond_map(const mcedm_ddpm_plan& P, const float* pk, const float* cond, float* map, int B, hipStream_t s) {
  const int R = P.desc.resolution;
  MCEDM_REQUIRE(B > 0 && B <= 65535, "ddpm_cond_map: batch %d outside [1, 65535]", B);
  hipLaunchKernelGGL(ddpm_cond_map_kernel, dim3(ceil_div(R, CM_PW), R, B), dim3(CM_NT), 0, s, cond, P.cond_channels, pk + P.enc0_w,
                     pk + P.enc0_b, pk + P.map_w, pk + P.map_b, P.desc.ch, R, map);
  MCEDM_LAUNCH_CHECK("ddpm_cond_map_kernel");
  return MCEDM_OK;
}

// ------------------------------------------------------------------------------------------
// forward schedule, written once and run twice: `dry` (sizes only) and for real
// ------------------------------------------------------------------------------------------
struct DT { int C = 0, H = 0, W = 0; size_t off = NONE, bytes = 0, sums = NONE, sums_bytes = 0; SumTiles st; int rc = 0; };

// Channels per fused-statistics record of a C-channel tensor: GroupNorm(32) consumes it alone with C / 32 channels per
// group (2 at C = 64: pair records; multiples of 4: quad records) or inside a concat whose groups are unions of those.
// 0: no fused statistics for this width (a gn_coef_kernel pass instead).
static int record_width(int C) {
  const int cpg = C / 32;
  return (C % 32) ? 0 : (cpg % 4 == 0) ? 4 : (cpg % 2 == 0) ? 2 : 0;
}

struct DExec {
  const mcedm_ddpm_plan& P;
  bool dry;
  char* base;                 // activation region
  const float* pk;
  hipStream_t s;
  int B;
  Pool pool;
  std::vector<DT> t;
  int bias_batch = 0;         // floats between the samples' row sets of the timestep table (one timestep per sample), 0: one set

  int act(int C, int H, int W, bool with_sums) {
    DT d; d.C = C; d.H = H; d.W = W;
    d.bytes = (size_t)B * C * H * W * sizeof(float);
    d.off = pool.alloc(d.bytes);
    d.rc = with_sums ? record_width(C) : 0;
    if (d.rc) {
      d.sums_bytes = (size_t)B * conv_max_tiles(H, W) * ceil_div(C, d.rc) * 2 * sizeof(float);
      d.sums = pool.alloc(d.sums_bytes);
    }
    t.push_back(d);
    return (int)t.size() - 1;
  }
  int raw(size_t bytes) { DT d; d.bytes = bytes; d.off = pool.alloc(bytes); t.push_back(d); return (int)t.size() - 1; }
  void release(int id) {
    if (id < 0) return;
    pool.release(t[id].off, t[id].bytes);
    if (t[id].sums != NONE) pool.release(t[id].sums, t[id].sums_bytes);
  }
  float* ptr(int id) const { return id < 0 ? nullptr : reinterpret_cast<float*>(base + t[id].off); }
  float* sums(int id) const { return (id < 0 || t[id].sums == NONE) ? nullptr : reinterpret_cast<float*>(base + t[id].sums); }
};

// conv `c` reads swish(GroupNorm(cat(xa, xb))): fused from the producers' statistics records when every group is a
// whole number of records of each source (pair records on the 64-channel tensors, quads on wider ones), else one pass
// of gn_coef_kernel into a table (returned id, to be released after the conv)
static int gn_into(DExec& E, const DNorm& n, int xa, int xb, ConvArgs& c, int* table_id) {
  const DT& A = E.t[xa];
  const int Ca = A.C, Cb = xb >= 0 ? E.t[xb].C : 0;
  GnArgs g{E.ptr(xa), E.ptr(xb), Ca, Cb, A.H * A.W, E.B, 32, E.pk + n.gamma, E.pk + n.beta, nullptr, 0, 0, E.P.desc.eps,
           nullptr, nullptr, E.sums(xa), E.sums(xb), A.st, xb >= 0 ? E.t[xb].st : SumTiles{}, A.W};
  *table_id = -1;
  c.act = 1; c.coef_batch = 1;
  const int cpg = (Ca + Cb) / 32, ra = A.rc, rb = xb >= 0 ? E.t[xb].rc : A.rc;
  const bool usable = (Ca + Cb) % 32 == 0 && ra > 0 && rb > 0 && cpg % ra == 0 && cpg % rb == 0 && Ca % ra == 0 && Ca % rb == 0;
  if (usable) {
    if (!E.dry && !gn_sums_usable(g)) { set_error("ddpm forward: statistics table of a %d-channel input is unusable", Ca + Cb); return MCEDM_ERR_INVALID; }
    c.gn = g; c.gn_on = 1; c.coef = nullptr;
    return MCEDM_OK;
  }
  *table_id = E.raw((size_t)E.B * (Ca + Cb) * sizeof(Coef));
  g.coef = reinterpret_cast<Coef*>(E.ptr(*table_id));
  c.coef = g.coef;
  return E.dry ? MCEDM_OK : launch_gn_coef(g, E.s);
}

static void src_of(const DExec& E, ConvArgs& c, int xa, int xb) {
  c.xa = E.ptr(xa); c.Ca = E.t[xa].C;
  c.xb = E.ptr(xb); c.Cb = xb >= 0 ? E.t[xb].C : 0;
  c.Hs = E.t[xa].H; c.Ws = E.t[xa].W; c.H = c.Hs; c.W = c.Ws;
}
static void dst_of(DExec& E, ConvArgs& c, int out, const DConv& cv, const float* bias, bool stats) {
  c.wpk = E.pk + cv.wpk; c.bias = bias ? bias : E.pk + cv.bias;
  // (below 32 x 32 the DDPM U-Net keeps its input-resident / tiled kernels: its conv1 has a bias row per sample in one entry and a
  // shared row in the other, the two must agree bit for bit, and the Winograd kernel's split variant has no per-sample form)
  c.wino = cv.wino != NONE && !conv_wino_small(E.t[out].H, E.t[out].W) ? E.pk + cv.wino : nullptr;
  c.out = E.ptr(out); c.Cout = cv.cout; c.B = E.B;
  if (stats && E.t[out].rc) { c.gsum = E.sums(out); c.gsum_rc = E.t[out].rc; c.gsum_tiles = &E.t[out].st; }
}
// the tiling a launch WOULD use must be known in the dry run too (the consumer's usability test reads st.tiles):
// the real launch overwrites it with the same values
static int run_conv(DExec& E, ConvArgs& c, int taps, int out) {
  if (E.dry) { if (c.gsum_tiles) *c.gsum_tiles = SumTiles{1, 1, 8, 8, c.gsum_rc == 2 ? 2 : 4}; (void)out; return MCEDM_OK; }
  return launch_conv(c, taps, E.s);
}

// ResnetBlock.forward (ddim_blocks.py:144-164) on cat(xa, xb); returns the output tensor id
static int res_block(DExec& E, const DRes& r, int xa, int xb, const float* bias_table, int* out_id) {
  const int bias_batch = E.bias_batch;                        // rows of bias_table per sample (0: one row set for the batch)
  int rc, tab;
  const int H = E.t[xa].H, W = E.t[xa].W;
  const int h = E.act(r.cout, H, W, true);
  ConvArgs c1{};
  src_of(E, c1, xa, xb);
  if ((rc = gn_into(E, r.n1, xa, xb, c1, &tab))) return rc;
  dst_of(E, c1, h, r.c1, bias_table + r.brow, true);          // bias = conv1.bias + temb_proj(swish(temb))
  c1.bias_batch = bias_batch;
  if ((rc = run_conv(E, c1, 9, h))) return rc;
  E.release(tab);
  // y = conv2(swish(norm2(h))) + (nin_shortcut(x) | x).  The 1x1 shortcut is a GEMM onto conv2's output tile, so it rides on
  // conv2 as extra K chunks at the centre tap (ConvArgs::sk_*, as the ADM decoder's skip projection does): the projected
  // tensor is neither written nor read back, one launch less per block
  const int y = E.act(r.cout, H, W, true);
  ConvArgs c2{};
  src_of(E, c2, h, -1);
  if ((rc = gn_into(E, r.n2, h, -1, c2, &tab))) return rc;
  dst_of(E, c2, y, r.c2, nullptr, true);
  int scid = -1;
  if (r.has_sc && r.c2.wino != NONE && conv_wino_shape_ok(r.cout, r.cout, H, W)) {
    // conv2 goes to the Winograd kernel, where a 1x1 projection cannot ride along: it runs as its own launch and enters
    // conv2 as the residual
    scid = E.act(r.cout, H, W, false);
    ConvArgs cs{};
    src_of(E, cs, xa, xb);
    dst_of(E, cs, scid, r.sc, nullptr, false);
    if ((rc = run_conv(E, cs, 1, scid))) return rc;
    c2.res = E.ptr(scid); c2.res_mode = RS_NONE;
  } else if (r.has_sc) {
    c2.sk_xa = E.ptr(xa); c2.sk_Ca = E.t[xa].C;
    c2.sk_xb = E.ptr(xb); c2.sk_Cb = xb >= 0 ? E.t[xb].C : 0;
    c2.sk_wpk = E.pk + r.sc.wpk; c2.sk_bias = E.pk + r.sc.bias;
  } else {
    c2.res = E.ptr(xa); c2.res_mode = RS_NONE;
  }
  if ((rc = run_conv(E, c2, 9, y))) return rc;
  E.release(tab);
  E.release(h);
  if (scid >= 0) E.release(scid);
  *out_id = y;
  return MCEDM_OK;
}

// AttnBlock.forward (ddim_blocks.py:194-219); consumes x (released here), returns the output id
static int attn_block(DExec& E, const DAttn& a, int x, int* out_id) {
  int rc, tab;
  const int H = E.t[x].H, W = E.t[x].W;
  const int qkv = E.act(3 * a.C, H, W, false);
  ConvArgs cq{};
  src_of(E, cq, x, -1);
  if ((rc = gn_into(E, a.n, x, -1, cq, &tab))) return rc;
  cq.act = 0;                                               // no nonlinearity between norm and q / k / v
  dst_of(E, cq, qkv, a.qkv, nullptr, false);
  if ((rc = run_conv(E, cq, 1, qkv))) return rc;
  E.release(tab);
  const int av = E.act(a.C, H, W, false);
  if (!E.dry && (rc = launch_attention(E.ptr(qkv), E.ptr(av), E.B, 1, H * W, E.s))) return rc;
  E.release(qkv);
  const int z = E.act(a.C, H, W, true);
  ConvArgs cp{};
  src_of(E, cp, av, -1);
  dst_of(E, cp, z, a.proj, nullptr, true);
  cp.res = E.ptr(x); cp.res_mode = RS_NONE;
  if ((rc = run_conv(E, cp, 1, z))) return rc;
  E.release(av);
  E.release(x);
  *out_id = z;
  return MCEDM_OK;
}

// header in front of the activations
struct DHeader { size_t bias, coef_in, F, Fu, total; };      // Fu: the guidance pass of a cat_cond plan (NONE otherwise)
static DHeader dheader(const mcedm_ddpm_plan& P, int B, int H, int W) {
  DHeader h;
  size_t cur = 0;
  auto take = [&](size_t bytes) { size_t o = cur; cur += align_up(bytes, 256); return o; };
  h.bias = take((size_t)P.rows * sizeof(float));
  h.coef_in = take((size_t)P.in_total * sizeof(Coef));
  h.F = take((size_t)B * P.desc.out_channels * H * W * sizeof(float));
  h.Fu = P.cat_channels > 0 ? take((size_t)B * P.desc.out_channels * H * W * sizeof(float)) : NONE;
  h.total = cur;
  return h;
}
static size_t state_floats(const mcedm_ddpm_plan& P, int B) {
  return (size_t)B * P.desc.in_channels * P.desc.resolution * P.desc.resolution;
}
static size_t map_bytes(const mcedm_ddpm_plan& P, int B) {
  return (size_t)B * P.desc.ch * P.desc.resolution * P.desc.resolution * sizeof(float);
}

// One evaluation's inputs.  The input is scaled by the rows of coef_in (null = identity) while conv_in stages it; cond enters
// as cond_map (null: None) on a plan with the head, as cond_cat [B, cat_channels, R, R] (null: None, zeros) on a cat_cond plan.
struct DdpmIn {
  const float* x = nullptr;
  float t = 0.f;
  const Coef* coef_in = nullptr;
  // one timestep per sample: t_dev [B] in device memory replaces t, and the rows go to rows_t [B][plan.rows] (the caller's, in front
  // of the network's region: the header keeps its one row set); coef_batch 1: coef_in holds a row set per sample
  const float* t_dev = nullptr;
  float* rows_t = nullptr;
  int coef_batch = 0;
  const float* self_cond = nullptr;
  const float* cond_map = nullptr;
  const float* cond_cat = nullptr;
};

// A plan bound to its packed weights, its region of a workspace (header, then activations), a batch size and a stream
struct DdpmNet {
  const mcedm_ddpm_plan* plan = nullptr;
  const float* pk = nullptr;
  DHeader hd{};
  char* ws = nullptr;         // start of the network's region
  int B = 0;
  hipStream_t s = nullptr;
  int ddpm_forward(bool dry, const DdpmIn& in, float* out, size_t* peak) const;      // the schedule; dry: sizes only
  int forward(const DdpmIn& in, float* out) const { return ddpm_forward(false, in, out, nullptr); }
  // F <- the network on `in`; Fu (unless null) <- the same without its conditioning: the two passes of classifier-free guidance
  int forward_cfg(DdpmIn in, float* F, float* Fu) const {
    const int rc = forward(in, F);
    if (rc || !Fu) return rc;
    in.cond_map = in.cond_cat = nullptr;
    return forward(in, Fu);
  }
  float* F() const { return at<float>(ws, hd.F); }
  float* Fu() const { return at<float>(ws, hd.Fu); }
  Coef* coef_in() const { return at<Coef>(ws, hd.coef_in); }
  // the rows of coef_in <- c_in on the state channels, identity on what conv_in reads in front of them
  int scale_input(float c_in) const { return launch_vp_coef(c_in, plan->in_total - plan->desc.in_channels, plan->desc.in_channels, coef_in(), s); }
  size_t state() const { return state_floats(*plan, B); }
};

// Model.forward (ddim_blocks.py:410-470) with dx None.  Returns the peak bytes of the activation region in *peak.
int DdpmNet::ddpm_forward(bool dry, const DdpmIn& in, float* out, size_t* peak) const {
  const mcedm_ddpm_plan& P = *plan;
  const mcedm_ddpm_desc& d = P.desc;
  const int R = d.resolution, L = d.n_levels;
  float* bias_table = dry ? nullptr : in.t_dev ? in.rows_t : at<float>(ws, hd.bias);
  int rc;
  if (!dry && in.t_dev) {
    if ((rc = launch_temb_rows(P, pk, in.t_dev, B, bias_table, s))) return rc;
  } else if (!dry) {
    int nsplit = P.rows / 32; if (nsplit < 1) nsplit = 1; if (nsplit > 64) nsplit = 64;
    const int ch = d.ch;
    hipLaunchKernelGGL(ddpm_temb_kernel, dim3(nsplit), dim3(TEMB_NT), (size_t)(ch + 8 * ch) * sizeof(float), s, in.t, ch, pk + P.freqs,
                       pk + P.w0, pk + P.b0, pk + P.w1, pk + P.b1, pk + P.tproj_w, pk + P.tproj_b, pk + P.c1bias, P.rows, bias_table);
    MCEDM_LAUNCH_CHECK("ddpm_temb_kernel");
  }
  DExec E{P, dry, dry ? nullptr : at<char>(ws, hd.total), pk, s, B, Pool(), {}};
  E.t.reserve(4096);        // ConvArgs::gsum_tiles points into this vector during a launch
  E.bias_batch = in.t_dev ? P.rows : 0;
  // conv_in on cat(x_self_cond = zeros, x): the self-conditioning half is a null source (reads as zeros); on a cat_cond plan
  // (no self-conditioning there) the first source is the conditioning instead, cat(cond, x)
  const int n_self = P.in_total - d.in_channels;
  const float* front = P.cat_channels > 0 ? in.cond_cat : in.self_cond;
  std::vector<int> hs;
  {
    const int h0 = E.act(d.ch, R, R, true);
    ConvArgs ci{};
    ci.xa = front; ci.Ca = n_self; ci.xb = in.x; ci.Cb = d.in_channels;          // a null first source reads as zeros
    if (n_self == 0) { ci.xa = in.x; ci.Ca = d.in_channels; ci.xb = nullptr; ci.Cb = 0; }
    ci.coef = in.coef_in; ci.coef_batch = in.coef_batch; ci.act = 0;
    ci.Hs = R; ci.Ws = R; ci.H = R; ci.W = R;
    dst_of(E, ci, h0, P.conv_in, nullptr, true);
    // the head: conv_in holds the folded weights; with cond the map (which carries its own bias) enters as the residual, in
    // front of the statistics; without it (cond None: zero features, not cond_enc(0)) the folded bias Wx b_in + b_comb alone
    if (in.cond_map) { ci.bias = nullptr; ci.res = in.cond_map; ci.res_mode = RS_NONE; }
    if ((rc = run_conv(E, ci, 9, h0))) return rc;
    hs.push_back(h0);
  }
  for (int l = 0; l < L; ++l) {
    const DLevel& lv = P.down[l];
    for (size_t j = 0; j < lv.blocks.size(); ++j) {
      int h;
      if ((rc = res_block(E, lv.blocks[j], hs.back(), -1, bias_table, &h))) return rc;
      if (!lv.attns.empty() && (rc = attn_block(E, lv.attns[j], h, &h))) return rc;
      hs.push_back(h);
    }
    if (lv.has_rs) {                                           // Downsample: stride-2 conv, no norm / activation
      const int src = hs.back();
      const int o = E.act(lv.rs.cout, E.t[src].H / 2, E.t[src].W / 2, true);
      ConvArgs cd{};
      src_of(E, cd, src, -1);
      cd.resample = RS_S2; cd.H = cd.Hs / 2; cd.W = cd.Ws / 2;
      dst_of(E, cd, o, lv.rs, nullptr, true);
      if ((rc = run_conv(E, cd, 9, o))) return rc;
      hs.push_back(o);
    }
  }
  // middle: hs[-1] stays on the stack (it is popped by the first up block)
  int h;
  if ((rc = res_block(E, P.mid1, hs.back(), -1, bias_table, &h))) return rc;
  if ((rc = attn_block(E, P.mid_attn, h, &h))) return rc;
  {
    int h2;
    if ((rc = res_block(E, P.mid2, h, -1, bias_table, &h2))) return rc;
    E.release(h);
    h = h2;
  }
  for (int l = L - 1; l >= 0; --l) {
    const DLevel& lv = P.up[l];
    for (size_t j = 0; j < lv.blocks.size(); ++j) {
      const int skip = hs.back(); hs.pop_back();
      int y;
      if ((rc = res_block(E, lv.blocks[j], h, skip, bias_table, &y))) return rc;     // cat([h, hs.pop()], dim=1)
      E.release(h); E.release(skip);
      h = y;
      if (!lv.attns.empty() && (rc = attn_block(E, lv.attns[j], h, &h))) return rc;
    }
    if (lv.has_rs) {                                           // Upsample: nearest 2x while staging, then 3x3
      const int o = E.act(lv.rs.cout, E.t[h].H * 2, E.t[h].W * 2, true);
      ConvArgs cu{};
      src_of(E, cu, h, -1);
      cu.resample = RS_UP; cu.H = cu.Hs * 2; cu.W = cu.Ws * 2;
      dst_of(E, cu, o, lv.rs, nullptr, true);
      if ((rc = run_conv(E, cu, 9, o))) return rc;
      E.release(h);
      h = o;
    }
  }
  MCEDM_REQUIRE(hs.empty(), "ddpm forward: %zu skip tensors left over", hs.size());
  // out = conv_out(swish(norm_out(h)))
  {
    int tab;
    ConvArgs co{};
    src_of(E, co, h, -1);
    if ((rc = gn_into(E, P.norm_out, h, -1, co, &tab))) return rc;
    co.wpk = pk + P.conv_out.wpk; co.bias = pk + P.conv_out.bias;
    co.out = out; co.Cout = d.out_channels; co.B = B;
    if (!dry && (rc = launch_conv(co, 9, s))) return rc;
    E.release(tab);
    E.release(h);
  }
  if (peak) *peak = E.pool.peak;
  return MCEDM_OK;
}

// *net <- (P, B, header offsets), *bytes <- what the network needs of a workspace: header + peak of the activations
static int ddpm_sizes(const mcedm_ddpm_plan& P, int B, DdpmNet* net, size_t* bytes) {
  MCEDM_REQUIRE(B > 0, "ddpm: empty batch");
  *net = DdpmNet{&P, nullptr, dheader(P, B, P.desc.resolution, P.desc.resolution), nullptr, B, nullptr};
  size_t act = 0;
  const int rc = net->ddpm_forward(true, DdpmIn{}, nullptr, &act);
  if (rc == MCEDM_OK) *bytes = net->hd.total + act;
  return rc;
}

// The one place that knows the workspace layout: `front_bytes` of the caller's own buffers (a sampler's), then the network's
// header and activations.  `who` names the entry in the message of a workspace that is too small.
static int ddpm_bind(const char* who, const mcedm_ddpm_plan& P, const void* packed, void* workspace, size_t workspace_bytes,
                     size_t front_bytes, int B, void* stream, DdpmNet* net) {
  int rc;
  size_t need = 0;
  if ((rc = ddpm_sizes(P, B, net, &need))) return rc;
  if ((rc = heun_check_workspace(who, workspace_bytes, front_bytes + need))) return rc;
  net->pk = (const float*)packed; net->ws = at<char>(workspace, front_bytes); net->s = (hipStream_t)stream;
  return MCEDM_OK;
}

// get_denoised (ddim.py:915-947): D = x + (-sigma) F(c_in x, c_noise), sigma and c_noise host scalars
static int ddpm_denoise_impl(const DdpmNet& net, const float* x, float sigma, float c_noise, float* D_out, float* F_out) {
  const mcedm_ddpm_plan& P = *net.plan;
  int rc;
  const float c_in = 1.0f / sqrtf(sigma * sigma + 1.0f);                 // 1 / (sigma ** 2 + 1).sqrt(), fp32
  DdpmIn in{x, c_noise};
  in.coef_in = net.coef_in();
  if ((rc = net.scale_input(c_in))) return rc;
  float* F = F_out ? F_out : net.F();
  if ((rc = net.forward(in, F))) return rc;
  const size_t total = (size_t)net.B * P.desc.out_channels * P.desc.resolution * P.desc.resolution;
  return launch_vp_finish(x, F, sigma, total, D_out, net.s);
}

// round_sigma (ddim.py:949-957): nearest entry of edm_steps in fp32; ties resolve to the lower index like argmin
static int nearest_step(const float* steps, int n, float sigma) {
  int best = 0;
  float bd = fabsf(sigma - steps[0]);
  for (int j = 1; j < n; ++j) {
    const float dd = fabsf(sigma - steps[j]);
    if (dd < bd) { bd = dd; best = j; }
  }
  return best;
}


// a size query: the caller's own buffers (bufs_of(plan, B).total bytes, a sampler's) in front of the network's workspace
template <class BufsOf>
static int workspace_query(const char* who, const mcedm_ddpm_plan* plan, int B, size_t* bytes, BufsOf bufs_of) {
  VariantScope variant_scope__(plan);
  MCEDM_REQUIRE(plan && bytes, "%s: null argument", who);
  DdpmNet net;
  const int rc = ddpm_sizes(*plan, B, &net, bytes);
  if (rc == MCEDM_OK) *bytes += bufs_of(*plan, B).total;
  return rc;
}

// what the four forward entries do behind their own argument checks
static int forward_entry(const char* who, const mcedm_ddpm_plan* plan, const void* packed, const DdpmIn& in, float* out,
                         void* workspace, size_t workspace_bytes, int B, void* stream) {
  DdpmNet net;
  const int rc = ddpm_bind(who, *plan, packed, workspace, workspace_bytes, 0, B, stream, &net);
  return rc ? rc : net.forward(in, out);
}
}  // namespace mcedm

extern "C" int mcedm_ddpm_workspace_bytes(const mcedm_ddpm_plan* plan, int B, size_t* bytes) {
  return workspace_query("ddpm_workspace_bytes", plan, B, bytes, [](const mcedm_ddpm_plan&, int) { return HeunBufs{}; });
}

extern "C" int mcedm_ddpm_forward(const mcedm_ddpm_plan* plan, const void* packed, const float* x, float t, float* out,
                                  void* workspace, size_t workspace_bytes, int B, void* stream) {
  VariantScope variant_scope__(plan);
  MCEDM_REQUIRE(plan && packed && x && out && workspace, "ddpm_forward: null argument");
  return forward_entry("ddpm_forward", plan, packed, DdpmIn{x, t}, out, workspace, workspace_bytes, B, stream);
}

extern "C" int mcedm_ddpm_forward_sc(const mcedm_ddpm_plan* plan, const void* packed, const float* x, const float* x_self_cond,
                                     float t, float* out, void* workspace, size_t workspace_bytes, int B, void* stream) {
  VariantScope variant_scope__(plan);
  MCEDM_REQUIRE(plan && packed && x && out && workspace, "ddpm_forward_sc: null argument");
  MCEDM_REQUIRE(!x_self_cond || plan->desc.self_cond, "ddpm_forward_sc: the network was built without self-conditioning channels");
  DdpmIn in{x, t};
  in.self_cond = x_self_cond;
  return forward_entry("ddpm_forward_sc", plan, packed, in, out, workspace, workspace_bytes, B, stream);
}

extern "C" int mcedm_ddpm_denoise(const mcedm_ddpm_plan* plan, const void* packed, const float* x, float sigma, float c_noise,
                                  float* D_out, float* F_out, void* workspace, size_t workspace_bytes, int B, void* stream) {
  VariantScope variant_scope__(plan);
  MCEDM_REQUIRE(plan && packed && x && D_out && workspace, "ddpm_denoise: null argument");
  DdpmNet net;
  const int rc = ddpm_bind("ddpm_denoise", *plan, packed, workspace, workspace_bytes, 0, B, stream, &net);
  return rc ? rc : ddpm_denoise_impl(net, x, sigma, c_noise, D_out, F_out);
}

namespace mcedm {
struct RBufs : HeunBufs { size_t mask; };
static RBufs rbufs(const mcedm_ddpm_plan& P, int B) {
  const size_t n = state_floats(P, B);
  RBufs r{heun_bufs(n), 0};
  r.mask = heun_take(r, n * 4);
  return r;
}
// hu_mask: 1 = known: rows [0, n_time_h) of the h channels and [0, n_time_u) of the u channels (ddim.py:970-972)
__global__ void repaint_mask_kernel(float* __restrict__ m, int C, int H, int W, int h_ch, int u_ch, int n_time_h, int n_time_u,
                                    size_t total) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int row = (int)((i / W) % H), c = (int)((i / ((size_t)W * H)) % C);
    float v = 1.0f;
    if (c < h_ch && row >= n_time_h) v = 0.0f;
    if (c >= h_ch && c < h_ch + u_ch && row >= n_time_u) v = 0.0f;
    m[i] = v;
  }
}
// m [B, C, R, R] <- the known-region mask of a sampler description's (h_ch, u_ch, n_time_h, n_time_u)
template <class Desc>
static int launch_repaint_mask(float* m, int C, int R, const Desc* sp, size_t total, hipStream_t s) {
  hipLaunchKernelGGL(repaint_mask_kernel, dim3(2048 < (total + 255) / 256 ? 2048 : (unsigned)((total + 255) / 256)), dim3(256), 0, s,
                     m, C, R, R, sp->h_ch, sp->u_ch, sp->n_time_h, sp->n_time_u, total);
  MCEDM_LAUNCH_CHECK("repaint_mask_kernel");
  return MCEDM_OK;
}
}  // namespace mcedm

extern "C" int mcedm_repaint_workspace_bytes(const mcedm_ddpm_plan* plan, int B, size_t* bytes) {
  return workspace_query("repaint_workspace_bytes", plan, B, bytes, rbufs);
}

extern "C" int mcedm_repaint_schedule(const mcedm_repaint_desc* sp, double* t_steps) {
  MCEDM_REQUIRE(sp && t_steps && sp->edm_steps && sp->num_diffusion_timesteps >= 2, "repaint_schedule: bad argument");
  MCEDM_REQUIRE(sp->timesteps >= 2, "repaint_schedule: timesteps=%d (the reference divides by timesteps-1)", sp->timesteps);
  const int n = sp->num_diffusion_timesteps, N = sp->timesteps;
  const double smin = std::max(sp->sigma_min, (double)sp->edm_steps[n - 1]);      // ddim.py:977-978 with :128-129
  const double smax = std::min(sp->sigma_max, (double)sp->edm_steps[0]);
  const double a = std::pow(smax, 1.0 / sp->rho), b = std::pow(smin, 1.0 / sp->rho) - std::pow(smax, 1.0 / sp->rho);
  for (int i = 0; i < N; ++i) {
    const double ts = std::pow(a + (double)i / (double)(N - 1) * b, sp->rho);
    t_steps[i] = (double)sp->edm_steps[nearest_step(sp->edm_steps, n, (float)ts)];      // round_sigma, ddim.py:986
  }
  t_steps[N] = 0.0;
  return MCEDM_OK;
}

namespace mcedm {
static int repaint_impl(const mcedm_ddpm_plan* plan, const void* packed, const mcedm_repaint_desc* sp, const float* hu,
                        const float* init_noise, const double* step_noise, const double* repeat_noise,
                        const unsigned long long* rng_seed, double* out, int return_last, void* workspace,
                        size_t workspace_bytes, int B, void* stream) {
  MCEDM_REQUIRE(plan && packed && sp && hu && init_noise && out && workspace, "repaint_sample: null argument");
  const mcedm_ddpm_plan& P = *plan;
  int rc;
  MCEDM_REQUIRE(P.desc.in_channels == P.desc.out_channels, "repaint_sample: in_channels != out_channels");
  MCEDM_REQUIRE(sp->edm_steps && sp->alphas_cumprod_ext && sp->num_diffusion_timesteps >= 2, "repaint_sample: missing schedule tables");
  MCEDM_REQUIRE(sp->timesteps >= 2 && sp->timesteps <= 4096 && sp->n_repeat >= 1, "repaint_sample: timesteps=%d n_repeat=%d out of range", sp->timesteps, sp->n_repeat);
  MCEDM_REQUIRE(sp->h_ch >= 0 && sp->u_ch >= 0 && sp->h_ch + sp->u_ch <= P.desc.in_channels, "repaint_sample: h_ch + u_ch exceeds the state channels");
  MCEDM_REQUIRE(std::fabs(sp->w) < 0.001, "repaint_sample: classifier-free guidance needs a conditional network (cond is None on this path, ddim.py:935)");
  MCEDM_REQUIRE(sp->n_repeat == 1 || repeat_noise != nullptr || rng_seed != nullptr, "repaint_sample: n_repeat > 1 needs repeat_noise");
  const int N = sp->timesteps, R = sp->n_repeat, n = sp->num_diffusion_timesteps;
  const int S = P.desc.resolution;
  std::vector<double> t(N + 1);
  if ((rc = mcedm_repaint_schedule(sp, t.data()))) return rc;
  const RBufs rb = rbufs(P, B);
  DdpmNet net;
  if ((rc = ddpm_bind("repaint_sample", P, packed, workspace, workspace_bytes, rb.total, B, stream, &net))) return rc;
  hipStream_t s = net.s;
  HeunState h = heun_state(workspace, rb, B, P.desc.in_channels, (size_t)S * S, N, return_last, out, s);
  float* mask = at<float>(workspace, rb.mask);
  const size_t total = h.total;

  auto alpha = [&](double tt) -> float {          // compute_alpha(t.long()) (ddim.py:700-704): the SIGMA is the index
    long idx = (long)tt + 1;
    if (idx < 0) idx = 0;
    if (idx > n) idx = n;
    return sp->alphas_cumprod_ext[idx];
  };
  auto round_sigma = [&](double sg) -> double { return (double)sp->edm_steps[nearest_step(sp->edm_steps, n, (float)sg)]; };
  auto denoise = [&](double sg, bool) -> int {    // get_denoised at a scalar sigma: c_noise = n - 1 - index(sigma)
    const float s32 = (float)sg;
    const float cn = (float)(n - 1 - nearest_step(sp->edm_steps, n, s32));
    return ddpm_denoise_impl(net, h.x32, s32, cn, h.D, nullptr);
  };

  if ((rc = launch_repaint_mask(mask, h.C, S, sp, total, s))) return rc;
  {
    const float aT = alpha(t[0]);
    if ((rc = launch_repaint_init(hu, init_noise, mask, sqrtf(aT), sqrtf(1.0f - aT), t[0], total, h.x, h.x32, s))) return rc;
  }
  if ((rc = heun_store_step(h, 0))) return rc;
  for (int i = 0; i < N; ++i) {
    const double t_cur = t[i], t_next = t[i + 1];
    const bool in_range = sp->S_min <= t_cur && t_cur <= sp->S_max;
    const double gamma = in_range ? std::min(sp->S_churn / N, std::sqrt(2.0) - 1.0) : 0.0;
    double t_hat = round_sigma(t_cur + gamma * t_cur);
    {
      const double c = std::sqrt(t_hat * t_hat - t_cur * t_cur) * sp->S_noise;          // ddim.py:1004
      if (c != 0.0) {
        MCEDM_REQUIRE(rng_seed != nullptr || step_noise != nullptr,
                      "repaint_sample: step %d adds noise (t_hat > t_cur) but step_noise is NULL", i);
        if ((rc = heun_churn(h, c, rng_seed ? nullptr : step_noise + (size_t)i * total, rng_seed, (unsigned long long)i * R,
                             nullptr))) return rc;
      }
    }
    for (int k = 0; k < R; ++k) {
      // Euler step (ddim.py:1008-1015) and 2nd order correction (:1018-1026); x holds x_hat, then x_next
      if ((rc = heun_update(h, i, t_hat, t_next, nullptr, denoise))) return rc;
      // replace the known part with the data noised to t_next (:1028-1031)
      const float at = alpha(t_next);
      if ((rc = launch_repaint_known(h.x, hu, init_noise, mask, sqrtf(at), sqrtf(1.0f - at), 0, total, h.x32, s))) return rc;
      if (k < R - 1) {                                                                   // back up from t_next to a new t_hat (:1033-1037)
        t_hat = round_sigma(t_next + (std::sqrt(2.0) - 1.0) * t_next);
        const double c = std::sqrt(t_hat * t_hat - t_next * t_next) * sp->S_noise;
        if ((rc = heun_churn(h, c, rng_seed ? nullptr : repeat_noise + ((size_t)i * (R - 1) + k) * total, rng_seed,
                             (unsigned long long)i * R + 1 + k, nullptr))) return rc;
      }
    }
    // :1041-1043
    if (i == N - 1 && (rc = launch_repaint_known(h.x, hu, init_noise, mask, 0.f, 0.f, 1, total, h.x32, s))) return rc;
    if ((rc = heun_store_step(h, i + 1))) return rc;
  }
  return heun_store_last(h);
}
}  // namespace mcedm

extern "C" int mcedm_repaint_sample(const mcedm_ddpm_plan* plan, const void* packed, const mcedm_repaint_desc* sp,
                                    const float* hu, const float* init_noise, const double* step_noise,
                                    const double* repeat_noise, double* out, int return_last, void* workspace,
                                    size_t workspace_bytes, int B, void* stream) {
  VariantScope variant_scope__(plan);
  return repaint_impl(plan, packed, sp, hu, init_noise, step_noise, repeat_noise, nullptr, out, return_last, workspace,
                      workspace_bytes, B, stream);
}
extern "C" int mcedm_repaint_sample_rng(const mcedm_ddpm_plan* plan, const void* packed, const mcedm_repaint_desc* sp,
                                        const float* hu, const float* init_noise, const uint64_t* rng_seed, double* out,
                                        int return_last, void* workspace, size_t workspace_bytes, int B, void* stream) {
  VariantScope variant_scope__(plan);
  MCEDM_REQUIRE(rng_seed != nullptr, "repaint_sample_rng: rng_seed is null");
  return repaint_impl(plan, packed, sp, hu, init_noise, nullptr, nullptr, reinterpret_cast<const unsigned long long*>(rng_seed),
                      out, return_last, workspace, workspace_bytes, B, stream);
}
extern "C" int mcedm_uniform_fill(float* out, size_t n, const uint64_t* rng_seed, uint64_t draw, void* stream) {
  MCEDM_REQUIRE(out && rng_seed, "uniform_fill: null argument");
  if (n == 0) return MCEDM_OK;
  return launch_uniform_fill(out, reinterpret_cast<const unsigned long long*>(rng_seed), draw, n, (hipStream_t)stream);
}
extern "C" int mcedm_normal_fill(double* out, size_t n, const uint64_t* rng_seed, uint64_t draw, void* stream) {
  MCEDM_REQUIRE(out && rng_seed, "normal_fill: null argument");
  if (n == 0) return MCEDM_OK;
  return launch_normal_fill(out, reinterpret_cast<const unsigned long long*>(rng_seed), draw, n, (hipStream_t)stream);
}

// ------------------------------------------------------------------------------------------
// PlDdim.sample_with_repeat (models/ddim.py:808-913): DDIM steps with RePaint inner loops, fp32 throughout
// ------------------------------------------------------------------------------------------
namespace mcedm {
struct DdimBufs { size_t xt, x0, et, mask, total; };
static DdimBufs ddim_bufs(const mcedm_ddpm_plan& P, int B) {
  DdimBufs r{};
  const size_t n = state_floats(P, B);
  r.xt = heun_take(r, n * 4); r.x0 = heun_take(r, n * 4); r.et = heun_take(r, n * 4); r.mask = heun_take(r, n * 4);
  return r;
}
}  // namespace mcedm

extern "C" int mcedm_ddim_workspace_bytes(const mcedm_ddpm_plan* plan, int B, size_t* bytes) {
  return workspace_query("ddim_workspace_bytes", plan, B, bytes, ddim_bufs);
}

// (the timestep sequence itself, ddim_timestep_seq, is shared with the conditional sampler: edm.hpp)
extern "C" int mcedm_ddim_timesteps(int num_diffusion_timesteps, int timesteps, int skip_type, int* seq, int capacity, int* count) {
  MCEDM_REQUIRE(count && num_diffusion_timesteps >= 2 && timesteps >= 1 && timesteps <= num_diffusion_timesteps,
                "ddim_timesteps: bad schedule (timesteps=%d of %d)", timesteps, num_diffusion_timesteps);
  MCEDM_REQUIRE(skip_type == 0 || skip_type == 1, "ddim_timesteps: skip_type must be 0 (uniform) or 1 (quad)");
  const std::vector<int> s = ddim_timestep_seq(num_diffusion_timesteps, timesteps, skip_type);
  *count = (int)s.size();
  if (seq) {
    MCEDM_REQUIRE(capacity >= (int)s.size(), "ddim_timesteps: capacity %d < %d entries", capacity, (int)s.size());
    for (size_t i = 0; i < s.size(); ++i) seq[i] = s[i];
  }
  return MCEDM_OK;
}

// eta_noise / rng_seed: the uniform draws of the stochastic steps, read from slice k or generated in the step kernel as draw k
static int ddim_repaint_impl(const mcedm_ddpm_plan* plan, const void* packed, const mcedm_ddim_desc* sp, const float* hu,
                             const float* init_noise, const float* eta_noise, const unsigned long long* rng_seed, float* xs_out,
                             float* x0_out, int return_last, void* workspace, size_t workspace_bytes, int B, void* stream) {
  MCEDM_REQUIRE(plan && packed && sp && hu && init_noise && xs_out && workspace, "ddim_repaint_sample: null argument");
  const mcedm_ddpm_plan& P = *plan;
  MCEDM_REQUIRE(P.desc.in_channels == P.desc.out_channels, "ddim_repaint_sample: in_channels != out_channels");
  const int n = sp->num_diffusion_timesteps, N = sp->timesteps, R = sp->n_repeat;
  MCEDM_REQUIRE(sp->alphas_cumprod_ext && n >= 2 && N >= 1 && N <= n && R >= 1, "ddim_repaint_sample: bad schedule (timesteps=%d of %d, n_repeat=%d)", N, n, R);
  MCEDM_REQUIRE(sp->skip_type == 0 || sp->skip_type == 1, "ddim_repaint_sample: skip_type must be 0 (uniform) or 1 (quad)");
  MCEDM_REQUIRE(sp->h_ch >= 0 && sp->u_ch >= 0 && sp->h_ch + sp->u_ch <= P.desc.in_channels, "ddim_repaint_sample: h_ch + u_ch exceeds the state channels");
  MCEDM_REQUIRE(!sp->self_cond || P.desc.self_cond, "ddim_repaint_sample: self-conditioning asked of a network built without it");
  const bool stochastic = std::fabs(sp->eta) > 1e-10;                   // ddim.py:884
  MCEDM_REQUIRE(!stochastic || eta_noise != nullptr || rng_seed != nullptr, "ddim_repaint_sample: eta != 0 needs eta_noise");
  // the timestep sequence (ddim.py:823-830) and its predecessor list (:845)
  std::vector<int> seq = ddim_timestep_seq(n, N, sp->skip_type);
  const int S = (int)seq.size();
  int rc;
  const DdimBufs db = ddim_bufs(P, B);
  DdpmNet net;
  if ((rc = ddpm_bind("ddim_repaint_sample", P, packed, workspace, workspace_bytes, db.total, B, stream, &net))) return rc;
  hipStream_t s = net.s;
  float* xt = at<float>(workspace, db.xt);
  float* x0 = at<float>(workspace, db.x0);
  float* et = at<float>(workspace, db.et);
  float* mask = at<float>(workspace, db.mask);
  const int res = P.desc.resolution, C = P.desc.in_channels;
  const size_t hw = (size_t)res * res, total = net.state();
  const int Txs = return_last ? 1 : S + 1, Tx0 = return_last ? 1 : S;
  auto alpha = [&](int t) -> float { return sp->alphas_cumprod_ext[t + 1]; };      // compute_alpha(t): index t + 1 (ddim.py:700-704)

  if ((rc = launch_repaint_mask(mask, C, res, sp, total, s))) return rc;
  {   // x = (hu * a[-1].sqrt() + hu_noise * (1 - a[-1]).sqrt()) * mask + hu_noise * (1 - mask)   (:837-838); a[-1] = alpha(n - 1)
    const float aT = alpha(n - 1);
    if ((rc = launch_ddim_init(hu, init_noise, mask, sqrtf(aT), sqrtf(1.0f - aT), total, xt, s))) return rc;
  }
  if (!return_last && (rc = launch_store_f32(xt, C, hw, 0, Txs, total, xs_out, s))) return rc;
  bool have_x0 = false;
  for (int step = 0; step < S; ++step) {
    const int i = seq[S - 1 - step], j = (S - 1 - step) > 0 ? seq[S - 2 - step] : -1;
    const float a_t = alpha(i), at_next = alpha(j);
    const float s0 = sqrtf(a_t), s1 = sqrtf(1.0f - a_t);
    for (int k = 0; k < R; ++k) {
      DdpmIn in{xt, (float)i};
      in.self_cond = (sp->self_cond && have_x0) ? x0 : nullptr;        // x_self_cond = x0_t if self_condition else None (:863)
      if ((rc = net.forward(in, et))) return rc;
      if ((rc = launch_ddim_x0(xt, et, hu, mask, s0, s1, k < R - 1 ? 1 : 0, total, x0, s))) return rc;
      have_x0 = true;
    }
    const DdimNoiseCoefs nc = ddim_noise_coefs(stochastic, sp->eta, a_t, at_next);
    const float c1 = nc.c1, c2 = nc.c2;
    if (stochastic && rng_seed) {
      if ((rc = launch_ddim_next_rng(x0, et, hu, init_noise, mask, rng_seed, (unsigned long long)step, sqrtf(at_next), c1, c2, total,
                                     xt, s))) return rc;
    } else if ((rc = launch_ddim_next(x0, et, hu, init_noise, mask, stochastic ? eta_noise + (size_t)step * total : nullptr,
                                      sqrtf(at_next), c1, c2, total, xt, s))) return rc;
    if (!return_last) {
      if ((rc = launch_store_f32(xt, C, hw, step + 1, Txs, total, xs_out, s))) return rc;
      if (x0_out && (rc = launch_store_f32(x0, C, hw, step, Tx0, total, x0_out, s))) return rc;
    }
  }
  if (return_last) {
    if ((rc = launch_store_f32(xt, C, hw, 0, 1, total, xs_out, s))) return rc;
    if (x0_out && (rc = launch_store_f32(x0, C, hw, 0, 1, total, x0_out, s))) return rc;
  }
  return MCEDM_OK;
}

extern "C" int mcedm_ddim_repaint_sample(const mcedm_ddpm_plan* plan, const void* packed, const mcedm_ddim_desc* sp,
                                         const float* hu, const float* init_noise, const float* eta_noise, float* xs_out,
                                         float* x0_out, int return_last, void* workspace, size_t workspace_bytes, int B,
                                         void* stream) {
  VariantScope variant_scope__(plan);
  return ddim_repaint_impl(plan, packed, sp, hu, init_noise, eta_noise, nullptr, xs_out, x0_out, return_last, workspace,
                           workspace_bytes, B, stream);
}

extern "C" int mcedm_ddim_repaint_sample_rng(const mcedm_ddpm_plan* plan, const void* packed, const mcedm_ddim_desc* sp,
                                             const float* hu, const float* init_noise, const uint64_t* rng_seed, float* xs_out,
                                             float* x0_out, int return_last, void* workspace, size_t workspace_bytes, int B,
                                             void* stream) {
  VariantScope variant_scope__(plan);
  MCEDM_REQUIRE(rng_seed != nullptr, "ddim_repaint_sample_rng: rng_seed (a 64-bit seed in device memory) is null");
  return ddim_repaint_impl(plan, packed, sp, hu, init_noise, nullptr, reinterpret_cast<const unsigned long long*>(rng_seed), xs_out,
                           x0_out, return_last, workspace, workspace_bytes, B, stream);
}

// ------------------------------------------------------------------------------------------
// the single-task model (PlCondDdim on Model): the head's entries and the two samplers of sampler.hip on this network
// ------------------------------------------------------------------------------------------
extern "C" int mcedm_ddpm_cond_map(const mcedm_ddpm_plan* plan, const void* packed, const float* cond, float* map_out, int B,
                                   void* stream) {
  VariantScope variant_scope__(plan);
  MCEDM_REQUIRE(plan && packed && map_out, "ddpm_cond_map: null argument");
  MCEDM_REQUIRE(plan->cond_channels > 0, "ddpm_cond_map: the plan was built without the cond_enc head (mcedm_ddpm_plan_create_cond)");
  MCEDM_REQUIRE(cond != nullptr, "ddpm_cond_map: cond is null on a plan with cond_channels=%d", plan->cond_channels);
  return launch_cond_map(*plan, (const float*)packed, cond, map_out, B, (hipStream_t)stream);
}

extern "C" int mcedm_ddpm_forward_cond(const mcedm_ddpm_plan* plan, const void* packed, const float* x, const float* x_self_cond,
                                       const float* cond_map, float t, float* out, void* workspace, size_t workspace_bytes, int B,
                                       void* stream) {
  VariantScope variant_scope__(plan);
  MCEDM_REQUIRE(plan && packed && x && out && workspace, "ddpm_forward_cond: null argument");
  MCEDM_REQUIRE(!x_self_cond || plan->desc.self_cond, "ddpm_forward_cond: the network was built without self-conditioning channels");
  MCEDM_REQUIRE(!cond_map || plan->cond_channels > 0, "ddpm_forward_cond: cond_map given to a plan built without the cond_enc head");
  DdpmIn in{x, t};
  in.self_cond = x_self_cond; in.cond_map = cond_map;
  return forward_entry("ddpm_forward_cond", plan, packed, in, out, workspace, workspace_bytes, B, stream);
}

namespace mcedm {
// what both samplers check of (plan, cond) and the map they compute once per call (null: cond None)
static int cond_sampler_check(const char* who, const mcedm_ddpm_plan& P, const float* cond, int cond_channels, int B) {
  MCEDM_REQUIRE(P.desc.in_channels == P.desc.out_channels, "%s: in_channels != out_channels", who);
  MCEDM_REQUIRE(B > 0, "%s: empty batch", who);
  MCEDM_REQUIRE(cond_channels == 0 || cond_channels == P.cond_channels, "%s: cond_channels %d is neither 0 nor the plan's %d", who,
                cond_channels, P.cond_channels);
  MCEDM_REQUIRE((cond != nullptr) == (cond_channels > 0), "%s: cond goes with cond_channels > 0 (and only with it)", who);
  return MCEDM_OK;
}

struct DVpBufs : HeunBufs { size_t map, Fu, dx, g; };
static DVpBufs dvp_bufs_of(const mcedm_ddpm_plan& P, int B, bool pde) {
  DVpBufs v{heun_bufs(state_floats(P, B)), 0, 0, 0, 0};
  v.map = heun_take(v, map_bytes(P, B));
  v.Fu = heun_take(v, state_floats(P, B) * 4);
  if (pde) { v.dx = heun_take(v, state_floats(P, B) * 4); v.g = heun_take(v, state_floats(P, B) * 4); }      // PDE guidance: gradient, Darcy scratch
  return v;
}
static DVpBufs dvp_bufs(const mcedm_ddpm_plan& P, int B) { return dvp_bufs_of(P, B, false); }
static DVpBufs dvp_guided_bufs(const mcedm_ddpm_plan& P, int B) { return dvp_bufs_of(P, B, true); }

// gd: PDE guidance, dx = get_dx_log_prob(h, D) after every get_denoised (:1576, 1589), h = plane 0 of cond
static int dvp_sample_impl(const mcedm_ddpm_plan* plan, const void* packed, const mcedm_vp_sampler_desc* sp, const mcedm_guidance_desc* gd,
                           const float* cond, const float* init_noise, const double* step_noise, const uint64_t* rng_seed, double* out,
                           int return_last, void* workspace, size_t workspace_bytes, int B, void* stream) {
  MCEDM_REQUIRE(plan && packed && sp && init_noise && out && workspace, "ddpm_vp_heun_sample: null argument");
  MCEDM_REQUIRE(!(step_noise && rng_seed), "ddpm_vp_heun_sample: step_noise and rng_seed are both given (at most one of them)");
  MCEDM_REQUIRE(sp->t_steps && sp->t_hat && sp->c_noise, "ddpm_vp_heun_sample: null schedule array");
  const mcedm_ddpm_plan& P = *plan;
  int rc;
  if ((rc = cond_sampler_check("ddpm_vp_heun_sample", P, cond, sp->cond_channels, B))) return rc;
  const int R = P.desc.resolution;
  if ((rc = guidance_check("ddpm_vp_heun_sample", gd, P.desc.in_channels, cond, sp->cond_channels, R, R))) return rc;
  if ((rc = vp_check_schedule(sp, step_noise, rng_seed))) return rc;
  const DVpBufs vb = dvp_bufs_of(P, B, gd != nullptr);
  DdpmNet net;
  if ((rc = ddpm_bind("ddpm_vp_heun_sample", P, packed, workspace, workspace_bytes, vb.total, B, stream, &net))) return rc;
  hipStream_t s = net.s;
  HeunState h = heun_state(workspace, vb, B, P.desc.in_channels, (size_t)R * R, sp->timesteps, return_last, out, s);
  float* map = cond ? at<float>(workspace, vb.map) : nullptr;
  if (map && (rc = launch_cond_map(P, net.pk, cond, map, B, s))) return rc;
  const bool guided = std::fabs(sp->w) >= 0.001 && map != nullptr;             // :937-942, the second evaluation without cond
  float* Fu = guided ? at<float>(workspace, vb.Fu) : nullptr;
  float* dxg = gd ? at<float>(workspace, vb.dx) : nullptr;
  float* gscratch = gd ? at<float>(workspace, vb.g) : nullptr;
  // get_denoised (:915-947): D = x + (-sigma) F(c_in x, c_noise, cond); cond itself is NOT scaled (cat_condition False, :932),
  // so one map serves every noise level; x_self_cond is None (get_self_cond_edm, :1603-1605)
  return vp_heun_loop(h, sp, init_noise, step_noise, rng_seed, [&](double sigma_d, float c_noise) -> int {
    int e;
    const float sigma = (float)sigma_d;                                   // t.to(torch.float32)
    const float c_in = 1.0f / sqrtf(sigma * sigma + 1.0f);                // 1 / (sigma ** 2 + 1).sqrt(), fp32
    DdpmIn in{h.x32, c_noise};
    in.coef_in = net.coef_in(); in.cond_map = map;
    if ((e = net.scale_input(c_in))) return e;
    if ((e = net.forward_cfg(in, net.F(), Fu))) return e;
    if ((e = launch_vp_cfg_finish(h.x32, net.F(), Fu, sp->w, sigma, h.total, h.D, s)) || !gd) return e;
    return guidance_dx(P.cond_channels, *gd, cond, h.D, dxg, gscratch, B, R, R, s);
  }, dxg, gd ? (float)gd->weight : 0.f);
}

struct DCondDdimBufs { size_t xt, xtn, F, Fu, sc, map, total, dx, g; };
static DCondDdimBufs dcond_ddim_bufs_of(const mcedm_ddpm_plan& P, int B, bool pde) {
  DCondDdimBufs b{};
  const size_t n = state_floats(P, B);
  b.xt = heun_take(b, n * 4); b.xtn = heun_take(b, n * 4); b.F = heun_take(b, n * 4); b.Fu = heun_take(b, n * 4);
  b.sc = heun_take(b, n * 4);
  b.map = heun_take(b, map_bytes(P, B));
  if (pde) { b.dx = heun_take(b, n * 4); b.g = heun_take(b, n * 4); }      // PDE guidance: gradient, Darcy scratch
  return b;
}
static DCondDdimBufs dcond_ddim_bufs(const mcedm_ddpm_plan& P, int B) { return dcond_ddim_bufs_of(P, B, false); }
static DCondDdimBufs dcond_ddim_guided_bufs(const mcedm_ddpm_plan& P, int B) { return dcond_ddim_bufs_of(P, B, true); }

// gd: PDE guidance, dx = get_dx_log_prob(h, xt) at every step's noisy state (:1501), h = plane 0 of cond
static int dcond_ddim_impl(const mcedm_ddpm_plan* plan, const void* packed, const mcedm_cond_ddim_desc* sp, const mcedm_guidance_desc* gd,
                           const float* cond, const float* init_noise, const float* eta_noise, const uint64_t* rng_seed, float* xs_out,
                           float* x0_out, int return_last, void* workspace, size_t workspace_bytes, int B, void* stream) {
  MCEDM_REQUIRE(plan && packed && sp && init_noise && xs_out && x0_out && workspace, "ddpm_cond_ddim_sample: null argument");
  MCEDM_REQUIRE(!(eta_noise && rng_seed), "ddpm_cond_ddim_sample: eta_noise and rng_seed are both given (at most one of them)");
  const mcedm_ddpm_plan& P = *plan;
  int rc;
  if ((rc = cond_sampler_check("ddpm_cond_ddim_sample", P, cond, sp->cond_channels, B))) return rc;
  MCEDM_REQUIRE(!sp->self_cond || P.desc.self_cond, "ddpm_cond_ddim_sample: self-conditioning asked of a network built without it");
  const int R = P.desc.resolution, C = P.desc.in_channels;
  if ((rc = guidance_check("ddpm_cond_ddim_sample", gd, C, cond, sp->cond_channels, R, R))) return rc;
  if ((rc = cond_ddim_check_schedule(sp, eta_noise, rng_seed))) return rc;
  const DCondDdimBufs cb = dcond_ddim_bufs_of(P, B, gd != nullptr);
  DdpmNet net;
  if ((rc = ddpm_bind("ddpm_cond_ddim_sample", P, packed, workspace, workspace_bytes, cb.total, B, stream, &net))) return rc;
  hipStream_t s = net.s;
  float* dxg = gd ? at<float>(workspace, cb.dx) : nullptr;
  float* gscratch = gd ? at<float>(workspace, cb.g) : nullptr;
  float* map = cond ? at<float>(workspace, cb.map) : nullptr;
  if (map && (rc = launch_cond_map(P, net.pk, cond, map, B, s))) return rc;
  const bool guided = cond_ddim_guided(sp);
  // x_self_cond of the next step = this step's x0 prediction, written by the step kernel (:1490, 1505); both passes read it
  float* sc = sp->self_cond ? at<float>(workspace, cb.sc) : nullptr;
  CondDdimLoop lp{C, (size_t)R * R, net.state(), at<float>(workspace, cb.xt), at<float>(workspace, cb.xtn),
                  at<float>(workspace, cb.F), guided ? at<float>(workspace, cb.Fu) : nullptr, sc, nullptr, C, 0};
  return cond_ddim_loop(sp, lp, init_noise, eta_noise, rng_seed, xs_out, x0_out, return_last, s, [&](const float* xt, float t, int step) -> int {
    DdpmIn in{xt, t};
    in.self_cond = step > 0 ? sc : nullptr; in.cond_map = map;            // x_self_cond None in the first step: zeros
    return net.forward_cfg(in, lp.F, lp.Fu);
  }, dxg, gd ? (float)gd->weight : 0.f, [&](const float* xt) -> int {
    return guidance_dx(P.cond_channels, *gd, cond, xt, dxg, gscratch, B, R, R, s);
  });
}
}  // namespace mcedm

extern "C" int mcedm_ddpm_vp_sampler_workspace_bytes(const mcedm_ddpm_plan* plan, int B, size_t* bytes) {
  return workspace_query("ddpm_vp_sampler_workspace_bytes", plan, B, bytes, dvp_bufs);
}
extern "C" int mcedm_ddpm_vp_heun_sample(const mcedm_ddpm_plan* plan, const void* packed, const mcedm_vp_sampler_desc* sp,
                                         const float* cond, const float* init_noise, const double* step_noise, double* out,
                                         int return_last, void* workspace, size_t workspace_bytes, int B, void* stream) {
  VariantScope variant_scope__(plan);
  return dvp_sample_impl(plan, packed, sp, nullptr, cond, init_noise, step_noise, nullptr, out, return_last, workspace, workspace_bytes, B,
                         stream);
}
extern "C" int mcedm_ddpm_vp_heun_sample_rng(const mcedm_ddpm_plan* plan, const void* packed, const mcedm_vp_sampler_desc* sp,
                                             const float* cond, const float* init_noise, const uint64_t* rng_seed, double* out,
                                             int return_last, void* workspace, size_t workspace_bytes, int B, void* stream) {
  VariantScope variant_scope__(plan);
  MCEDM_REQUIRE(rng_seed != nullptr, "ddpm_vp_heun_sample_rng: rng_seed (a 64-bit seed in device memory) is null");
  return dvp_sample_impl(plan, packed, sp, nullptr, cond, init_noise, nullptr, rng_seed, out, return_last, workspace, workspace_bytes, B,
                         stream);
}
extern "C" int mcedm_ddpm_vp_guided_workspace_bytes(const mcedm_ddpm_plan* plan, int B, size_t* bytes) {
  return workspace_query("ddpm_vp_guided_workspace_bytes", plan, B, bytes, dvp_guided_bufs);
}
extern "C" int mcedm_ddpm_vp_heun_sample_guided(const mcedm_ddpm_plan* plan, const void* packed, const mcedm_vp_sampler_desc* sp,
                                                const mcedm_guidance_desc* gd, const float* cond, const float* init_noise,
                                                const double* step_noise, const uint64_t* rng_seed, double* out, int return_last,
                                                void* workspace, size_t workspace_bytes, int B, void* stream) {
  VariantScope variant_scope__(plan);
  return dvp_sample_impl(plan, packed, sp, gd, cond, init_noise, step_noise, rng_seed, out, return_last, workspace, workspace_bytes, B,
                         stream);
}

extern "C" int mcedm_ddpm_cond_ddim_workspace_bytes(const mcedm_ddpm_plan* plan, int B, size_t* bytes) {
  return workspace_query("ddpm_cond_ddim_workspace_bytes", plan, B, bytes, dcond_ddim_bufs);
}
extern "C" int mcedm_ddpm_cond_ddim_sample(const mcedm_ddpm_plan* plan, const void* packed, const mcedm_cond_ddim_desc* sp,
                                           const float* cond, const float* init_noise, const float* eta_noise, float* xs_out,
                                           float* x0_out, int return_last, void* workspace, size_t workspace_bytes, int B,
                                           void* stream) {
  VariantScope variant_scope__(plan);
  return dcond_ddim_impl(plan, packed, sp, nullptr, cond, init_noise, eta_noise, nullptr, xs_out, x0_out, return_last, workspace,
                         workspace_bytes, B, stream);
}
extern "C" int mcedm_ddpm_cond_ddim_sample_rng(const mcedm_ddpm_plan* plan, const void* packed, const mcedm_cond_ddim_desc* sp,
                                               const float* cond, const float* init_noise, const uint64_t* rng_seed, float* xs_out,
                                               float* x0_out, int return_last, void* workspace, size_t workspace_bytes, int B,
                                               void* stream) {
  VariantScope variant_scope__(plan);
  MCEDM_REQUIRE(rng_seed != nullptr, "ddpm_cond_ddim_sample_rng: rng_seed (a 64-bit seed in device memory) is null");
  return dcond_ddim_impl(plan, packed, sp, nullptr, cond, init_noise, nullptr, rng_seed, xs_out, x0_out, return_last, workspace,
                         workspace_bytes, B, stream);
}
extern "C" int mcedm_ddpm_cond_ddim_guided_workspace_bytes(const mcedm_ddpm_plan* plan, int B, size_t* bytes) {
  return workspace_query("ddpm_cond_ddim_guided_workspace_bytes", plan, B, bytes, dcond_ddim_guided_bufs);
}
extern "C" int mcedm_ddpm_cond_ddim_sample_guided(const mcedm_ddpm_plan* plan, const void* packed, const mcedm_cond_ddim_desc* sp,
                                                  const mcedm_guidance_desc* gd, const float* cond, const float* init_noise,
                                                  const float* eta_noise, const uint64_t* rng_seed, float* xs_out, float* x0_out,
                                                  int return_last, void* workspace, size_t workspace_bytes, int B, void* stream) {
  VariantScope variant_scope__(plan);
  return dcond_ddim_impl(plan, packed, sp, gd, cond, init_noise, eta_noise, rng_seed, xs_out, x0_out, return_last, workspace,
                         workspace_bytes, B, stream);
}

// ------------------------------------------------------------------------------------------
// the single-task EDM model (PlCondEdm on Model, configs/model/edm_cond_h_res32.yaml): cat_cond input, EDM preconditioning
// (models/ddim.py:1745-1763) and the Heun sampler (:1532-1601) with optional PDE guidance
// ------------------------------------------------------------------------------------------
namespace mcedm {
// cond goes with a cat_cond plan (NULL: cond None, zeros)
static int cat_check(const char* who, const mcedm_ddpm_plan& P, const float* cond, int B) {
  MCEDM_REQUIRE(B > 0, "%s: empty batch", who);
  MCEDM_REQUIRE(!cond || P.cat_channels > 0, "%s: cond given to a plan built without cat_cond channels (mcedm_ddpm_plan_create_cond)", who);
  return MCEDM_OK;
}

// get_denoised (:1745-1763) at one noise level, fp32 like the reference: c_in scales the state rows of conv_in only (cond is
// concatenated unscaled), F = (1 + w) F(cond) - w F(None) for |w| >= 1e-3 with cond given, D = c_skip x + c_out F
static int dedm_denoise_impl(const DdpmNet& net, const float* x, const float* cond, float sigma, float c_noise, double w,
                             float sigma_data, float* D_out, float* F_out) {
  int rc;
  const float sd2 = sigma_data * sigma_data, s2 = sigma * sigma;
  const float c_skip = sd2 / (s2 + sd2);
  const float c_out = sigma * sigma_data / sqrtf(s2 + sd2);
  const float c_in = 1.0f / sqrtf(sd2 + s2);
  DdpmIn in{x, c_noise};
  in.coef_in = net.coef_in(); in.cond_cat = cond;
  if ((rc = net.scale_input(c_in))) return rc;
  float* Fu = std::fabs(w) >= 0.001 && cond != nullptr ? net.Fu() : nullptr;
  if ((rc = net.forward_cfg(in, net.F(), Fu))) return rc;
  return launch_edm_cfg_finish(x, net.F(), Fu, w, c_skip, c_out, net.state(), D_out, F_out, net.s);
}

struct DEdmBufs : HeunBufs { size_t dx, g; };
static DEdmBufs dedm_bufs(const mcedm_ddpm_plan& P, int B) {
  DEdmBufs v{heun_bufs(state_floats(P, B)), 0, 0};
  v.dx = heun_take(v, state_floats(P, B) * 4); v.g = heun_take(v, state_floats(P, B) * 4);      // PDE guidance: gradient, Darcy scratch
  return v;
}

static int dedm_sample_impl(const mcedm_ddpm_plan* plan, const void* packed, const mcedm_vp_sampler_desc* sp, double sigma_data,
                            const mcedm_guidance_desc* gd, const float* cond, const float* init_noise, const double* step_noise,
                            const uint64_t* rng_seed, double* out, int return_last, void* workspace, size_t workspace_bytes, int B,
                            void* stream) {
  MCEDM_REQUIRE(plan && packed && sp && init_noise && out && workspace, "ddpm_edm_heun_sample: null argument");
  MCEDM_REQUIRE(sp->t_steps && sp->t_hat && sp->c_noise, "ddpm_edm_heun_sample: null schedule array");
  const mcedm_ddpm_plan& P = *plan;
  int rc;
  MCEDM_REQUIRE(P.desc.in_channels == P.desc.out_channels, "ddpm_edm_heun_sample: in_channels != out_channels");
  if ((rc = cat_check("ddpm_edm_heun_sample", P, cond, B))) return rc;
  MCEDM_REQUIRE(sp->cond_channels == (cond ? P.cat_channels : 0), "ddpm_edm_heun_sample: cond_channels %d, expected %d (the plan's with cond, 0 without)",
                sp->cond_channels, cond ? P.cat_channels : 0);
  MCEDM_REQUIRE(sigma_data > 0.0, "ddpm_edm_heun_sample: sigma_data %g <= 0", sigma_data);
  MCEDM_REQUIRE(gd == nullptr || gd->system == 1 || gd->system == 2, "ddpm_edm_heun_sample: guidance system must be 1 (SWE) or 2 (Darcy)");
  MCEDM_REQUIRE(gd == nullptr || (P.desc.in_channels == 1 && cond != nullptr),
                "ddpm_edm_heun_sample: PDE guidance is defined for the single-task sampler (state u, conditioning h in cond[:, 0]), "
                "models/ddim.py:1532-1601");
  if ((rc = vp_check_schedule(sp, step_noise, rng_seed))) return rc;
  const DEdmBufs eb = dedm_bufs(P, B);
  DdpmNet net;
  if ((rc = ddpm_bind("ddpm_edm_heun_sample", P, packed, workspace, workspace_bytes, eb.total, B, stream, &net))) return rc;
  hipStream_t s = net.s;
  const int R = P.desc.resolution;
  HeunState h = heun_state(workspace, eb, B, P.desc.in_channels, (size_t)R * R, sp->timesteps, return_last, out, s);
  float* dxg = gd ? at<float>(workspace, eb.dx) : nullptr;
  float* gscratch = at<float>(workspace, eb.g);
  const float sd = (float)sigma_data;
  // x_self_cond is None in every evaluation (no self-conditioning on a cat_cond plan); guidance: dx = get_dx_log_prob(h, D) after
  // each denoiser call (:1576, 1589)
  return vp_heun_loop(h, sp, init_noise, step_noise, rng_seed, [&](double sigma_d, float c_noise) -> int {
    int e = dedm_denoise_impl(net, h.x32, cond, (float)sigma_d, c_noise, sp->w, sd, h.D, nullptr);      // t.to(torch.float32)
    if (e || !gd) return e;
    return guidance_dx(P.cat_channels, *gd, cond, h.D, dxg, gscratch, B, R, R, s);
  }, dxg, gd ? (float)gd->weight : 0.f);
}
}  // namespace mcedm

extern "C" int mcedm_ddpm_forward_cat(const mcedm_ddpm_plan* plan, const void* packed, const float* x, const float* cond, float t,
                                      float* out, void* workspace, size_t workspace_bytes, int B, void* stream) {
  VariantScope variant_scope__(plan);
  MCEDM_REQUIRE(plan && packed && x && out && workspace, "ddpm_forward_cat: null argument");
  int rc;
  if ((rc = cat_check("ddpm_forward_cat", *plan, cond, B))) return rc;
  DdpmIn in{x, t};
  in.cond_cat = cond;
  return forward_entry("ddpm_forward_cat", plan, packed, in, out, workspace, workspace_bytes, B, stream);
}

extern "C" int mcedm_ddpm_edm_denoise(const mcedm_ddpm_plan* plan, const void* packed, const float* x, const float* cond, float sigma,
                                      float c_noise, double w, double sigma_data, float* D_out, float* F_out, void* workspace,
                                      size_t workspace_bytes, int B, void* stream) {
  VariantScope variant_scope__(plan);
  MCEDM_REQUIRE(plan && packed && x && D_out && workspace, "ddpm_edm_denoise: null argument");
  MCEDM_REQUIRE(sigma > 0.f && sigma_data > 0.0, "ddpm_edm_denoise: sigma %g and sigma_data %g must be positive", (double)sigma, sigma_data);
  int rc;
  if ((rc = cat_check("ddpm_edm_denoise", *plan, cond, B))) return rc;
  DdpmNet net;
  if ((rc = ddpm_bind("ddpm_edm_denoise", *plan, packed, workspace, workspace_bytes, 0, B, stream, &net))) return rc;
  return dedm_denoise_impl(net, x, cond, sigma, c_noise, w, (float)sigma_data, D_out, F_out);
}

extern "C" int mcedm_ddpm_edm_sampler_workspace_bytes(const mcedm_ddpm_plan* plan, int B, size_t* bytes) {
  return workspace_query("ddpm_edm_sampler_workspace_bytes", plan, B, bytes, dedm_bufs);
}
extern "C" int mcedm_ddpm_edm_heun_sample(const mcedm_ddpm_plan* plan, const void* packed, const mcedm_vp_sampler_desc* sp,
                                          double sigma_data, const mcedm_guidance_desc* gd, const float* cond, const float* init_noise,
                                          const double* step_noise, double* out, int return_last, void* workspace,
                                          size_t workspace_bytes, int B, void* stream) {
  VariantScope variant_scope__(plan);
  return dedm_sample_impl(plan, packed, sp, sigma_data, gd, cond, init_noise, step_noise, nullptr, out, return_last, workspace,
                          workspace_bytes, B, stream);
}
extern "C" int mcedm_ddpm_edm_heun_sample_rng(const mcedm_ddpm_plan* plan, const void* packed, const mcedm_vp_sampler_desc* sp,
                                              double sigma_data, const mcedm_guidance_desc* gd, const float* cond,
                                              const float* init_noise, const uint64_t* rng_seed, double* out, int return_last,
                                              void* workspace, size_t workspace_bytes, int B, void* stream) {
  VariantScope variant_scope__(plan);
  MCEDM_REQUIRE(rng_seed != nullptr, "ddpm_edm_heun_sample_rng: rng_seed (a 64-bit seed in device memory) is null");
  return dedm_sample_impl(plan, packed, sp, sigma_data, gd, cond, init_noise, nullptr, rng_seed, out, return_last, workspace,
                          workspace_bytes, B, stream);
}

// ------------------------------------------------------------------------------------------
// one timestep (noise level) per sample: what the noising pass of training evaluates (models/ddim.py:195-226, 1654-1694).  Every
// ResnetBlock's conv1 reads its own row set of the timestep table (ConvArgs::bias_batch); the table [B][rows], and for the EDM entry
// conv_in's transform rows [B][in_total] and c_noise [B], sit in front of the network's region, whose layout does not change.
// ------------------------------------------------------------------------------------------
namespace mcedm {
struct DTBufs { size_t rows, coef, c_noise, total; };
static DTBufs dt_bufs(const mcedm_ddpm_plan& P, int B) {
  DTBufs b{};
  b.rows = heun_take(b, (size_t)B * P.rows * sizeof(float));
  b.coef = heun_take(b, (size_t)B * P.in_total * sizeof(Coef));
  b.c_noise = heun_take(b, (size_t)B * sizeof(float));
  return b;
}
}  // namespace mcedm

extern "C" int mcedm_ddpm_temb_row_count(const mcedm_ddpm_plan* plan, int* rows) {
  MCEDM_REQUIRE(plan && rows, "ddpm_temb_row_count: null argument");
  *rows = plan->rows;
  return MCEDM_OK;
}

extern "C" int mcedm_ddpm_temb_rows(const mcedm_ddpm_plan* plan, const void* packed, const float* t, int B, float* rows_out,
                                    void* stream) {
  MCEDM_REQUIRE(plan && packed && t && rows_out, "ddpm_temb_rows: null argument");
  return launch_temb_rows(*plan, (const float*)packed, t, B, rows_out, (hipStream_t)stream);
}

extern "C" int mcedm_ddpm_workspace_bytes_t(const mcedm_ddpm_plan* plan, int B, size_t* bytes) {
  return workspace_query("ddpm_workspace_bytes_t", plan, B, bytes, dt_bufs);
}

extern "C" int mcedm_ddpm_forward_t(const mcedm_ddpm_plan* plan, const void* packed, const float* x, const float* x_self_cond,
                                    const float* cond_map, const float* cond_cat, const float* t, float* out, void* workspace,
                                    size_t workspace_bytes, int B, void* stream) {
  VariantScope variant_scope__(plan);
  MCEDM_REQUIRE(plan && packed && x && t && out && workspace, "ddpm_forward_t: null argument");
  MCEDM_REQUIRE(B > 0 && B <= 65535, "ddpm_forward_t: batch %d outside [1, 65535]", B);
  MCEDM_REQUIRE(!x_self_cond || plan->desc.self_cond, "ddpm_forward_t: the network was built without self-conditioning channels");
  MCEDM_REQUIRE(!cond_map || plan->cond_channels > 0, "ddpm_forward_t: cond_map given to a plan built without the cond_enc head");
  MCEDM_REQUIRE(!cond_cat || plan->cat_channels > 0, "ddpm_forward_t: cond_cat given to a plan built without cat_cond channels (mcedm_ddpm_plan_create_cond)");
  const DTBufs tb = dt_bufs(*plan, B);
  DdpmNet net;
  int rc;
  if ((rc = ddpm_bind("ddpm_forward_t", *plan, packed, workspace, workspace_bytes, tb.total, B, stream, &net))) return rc;
  DdpmIn in{x};
  in.self_cond = x_self_cond; in.cond_map = cond_map; in.cond_cat = cond_cat;
  in.t_dev = t; in.rows_t = at<float>(workspace, tb.rows);
  return net.forward(in, out);
}

extern "C" int mcedm_ddpm_edm_denoise_t(const mcedm_ddpm_plan* plan, const void* packed, const float* x, const float* cond,
                                        const float* sigma, double sigma_data, float* D_out, float* F_out, void* workspace,
                                        size_t workspace_bytes, int B, void* stream) {
  VariantScope variant_scope__(plan);
  MCEDM_REQUIRE(plan && packed && x && sigma && D_out && workspace, "ddpm_edm_denoise_t: null argument");
  MCEDM_REQUIRE(B > 0 && B <= 65535, "ddpm_edm_denoise_t: batch %d outside [1, 65535]", B);
  MCEDM_REQUIRE(sigma_data > 0.0, "ddpm_edm_denoise_t: sigma_data %g must be positive", sigma_data);
  MCEDM_REQUIRE(plan->desc.in_channels == plan->desc.out_channels, "ddpm_edm_denoise_t: in_channels != out_channels");
  int rc;
  if ((rc = cat_check("ddpm_edm_denoise_t", *plan, cond, B))) return rc;
  const DTBufs tb = dt_bufs(*plan, B);
  DdpmNet net;
  if ((rc = ddpm_bind("ddpm_edm_denoise_t", *plan, packed, workspace, workspace_bytes, tb.total, B, stream, &net))) return rc;
  const mcedm_ddpm_plan& P = *plan;
  Coef* coef = at<Coef>(workspace, tb.coef);
  float* c_noise = at<float>(workspace, tb.c_noise);
  const float sd = (float)sigma_data;
  if ((rc = launch_edm_prepare_t(sigma, sd, P.in_total - P.desc.in_channels, P.desc.in_channels, B, coef, c_noise, net.s))) return rc;
  DdpmIn in{x};
  in.coef_in = coef; in.coef_batch = 1; in.cond_cat = cond;
  in.t_dev = c_noise; in.rows_t = at<float>(workspace, tb.rows);
  if ((rc = net.forward(in, net.F()))) return rc;
  return launch_edm_finish_t(x, net.F(), sigma, sd, net.state() / B, net.state(), D_out, F_out, net.s);
}
