// ops_api.hip -- kernel-level C entry points (tests, per-kernel timing).
#include "common.hpp"
#include "conv_wino.hpp"
#include "bwd.hpp"
#include "edm.hpp"

using namespace mcedm;

static_assert(sizeof(mcedm_coef) == sizeof(Coef), "mcedm_coef must mirror Coef");

extern "C" size_t mcedm_op_conv_packed_floats(int Cout, int Cin, int k) {
  if (Cout <= 0 || Cin <= 0 || (k != 1 && k != 3)) return 0;
  return conv_packed_floats(Cout, Cin, k * k);
}

extern "C" int mcedm_op_pack_conv(const float* w, const float* b, int Cout, int Cin, int k, int qkv_heads, int dgrad,
                                  float* wpk, float* bias_pk, void* stream) {
  MCEDM_REQUIRE(w && wpk, "op_pack_conv: null pointer");
  MCEDM_REQUIRE(Cout > 0 && Cin > 0 && (k == 1 || k == 3), "op_pack_conv: bad shape");
  MCEDM_REQUIRE(qkv_heads == 0 || (Cout % (3 * qkv_heads) == 0 && !dgrad), "op_pack_conv: bad qkv_heads");
  int rc = dgrad ? launch_pack_conv(w, wpk, Cin, Cout, k * k, 0, 1, (hipStream_t)stream)
                 : launch_pack_conv(w, wpk, Cout, Cin, k * k, qkv_heads, 0, (hipStream_t)stream);
  if (rc) return rc;
  if (b && bias_pk) rc = launch_pack_bias(b, bias_pk, Cout, qkv_heads, (hipStream_t)stream);
  return rc;
}

extern "C" int mcedm_op_gn_coef(const float* xa, const float* xb, int Ca, int Cb, int B, int HW, const float* gamma,
                                const float* beta, const float* film, int film_batch, int film_stride, float eps,
                                mcedm_coef* coef_out, float* stats_out, void* stream) {
  MCEDM_REQUIRE(xa && gamma && beta && coef_out, "op_gn_coef: null pointer");
  MCEDM_REQUIRE(B > 0 && HW > 0 && Ca > 0 && Cb >= 0, "op_gn_coef: bad shape");
  const int C = Ca + Cb;
  MCEDM_REQUIRE(C >= 4, "op_gn_coef: C=%d < 4 gives zero groups (adm_blocks.py:89)", C);
  GnArgs a{xa, xb, Ca, Cb, HW, B, C / 4 < 32 ? C / 4 : 32, gamma, beta, film, film_batch, film_stride, eps,
           reinterpret_cast<Coef*>(coef_out), stats_out, nullptr, nullptr, SumTiles{}, SumTiles{}, 0};
  return launch_gn_coef(a, (hipStream_t)stream);
}

static int op_conv(const float* xa, const float* xb, int Ca, int Cb, const mcedm_coef* coef, int coef_batch, int act, int resample,
                   int Hs, int Ws, int H, int W, const float* wpk, const float* bias_pk, int bias_batch, const float* res, int res_mode,
                   float* out, int Cout, int B, int k, void* stream) {
  MCEDM_REQUIRE(k == 1 || k == 3, "op_conv: k must be 1 or 3");
  MCEDM_REQUIRE(resample >= 0 && resample <= 3 && res_mode >= 0 && res_mode <= 2, "op_conv: bad resample mode");
  ConvArgs a{};
  a.xa = xa; a.xb = xb; a.Ca = Ca; a.Cb = Cb;
  a.coef = reinterpret_cast<const Coef*>(coef); a.coef_batch = coef_batch; a.act = act;
  a.resample = resample; a.Hs = Hs; a.Ws = Ws; a.H = H; a.W = W;
  a.wpk = wpk; a.bias = bias_pk; a.res = res; a.res_mode = res_mode;
  a.out = out; a.Cout = Cout; a.B = B; a.bias_batch = bias_batch;
  return launch_conv(a, k * k, (hipStream_t)stream);
}
extern "C" int mcedm_op_conv(const float* xa, const float* xb, int Ca, int Cb, const mcedm_coef* coef, int coef_batch,
                             int act, int resample, int Hs, int Ws, int H, int W, const float* wpk,
                             const float* bias_pk, const float* res, int res_mode, float* out, int Cout, int B, int k,
                             void* stream) {
  return op_conv(xa, xb, Ca, Cb, coef, coef_batch, act, resample, Hs, Ws, H, W, wpk, bias_pk, 0, res, res_mode, out, Cout, B, k, stream);
}
// mcedm_op_conv with a bias row per sample: bias_pk [B][bias_batch] (each row in packed order); a launcher whose kernel does not
// implement it refuses a non-zero bias_batch
extern "C" int mcedm_op_conv_bias_batch(const float* xa, const float* xb, int Ca, int Cb, const mcedm_coef* coef, int coef_batch,
                                        int act, int resample, int Hs, int Ws, int H, int W, const float* wpk, const float* bias_pk,
                                        int bias_batch, const float* res, int res_mode, float* out, int Cout, int B, int k,
                                        void* stream) {
  MCEDM_REQUIRE(bias_batch >= 0, "op_conv_bias_batch: bias_batch %d < 0", bias_batch);
  return op_conv(xa, xb, Ca, Cb, coef, coef_batch, act, resample, Hs, Ws, H, W, wpk, bias_pk, bias_batch, res, res_mode, out, Cout, B, k,
                 stream);
}

extern "C" size_t mcedm_op_conv_wino_packed_floats(int Cout, int Cin) { return conv_wino_packed_floats(Cout, Cin); }

extern "C" int mcedm_op_pack_conv_wino(const float* w, int Cout, int Cin, float* wino, void* stream) {
  return launch_pack_conv_wino(w, wino, Cout, Cin, 0, (hipStream_t)stream);
}

// the table backward.hip feeds into conv_wino_kernel for a 3x3 data gradient (plan.hip: the plan's dgrad tables)
extern "C" int mcedm_op_pack_conv_wino_dgrad(const float* w, int Cout, int Cin, float* wino, void* stream) {
  return launch_pack_conv_wino(w, wino, Cin, Cout, 1, (hipStream_t)stream);
}

extern "C" int mcedm_op_conv_wino(const float* xa, const float* xb, int Ca, int Cb, const mcedm_coef* coef, int coef_batch,
                                  int act, int resample, int H, int W, const float* wino, const float* bias, const float* res,
                                  int res_mode, float* out, int Cout, int B, void* stream) {
  MCEDM_REQUIRE((resample == RS_NONE || resample == RS_UP) && (res_mode == RS_NONE || res_mode == RS_UP || res_mode == RS_DOWN),
                "op_conv_wino: resample must be 0 (none) or 1 (nearest-2x up), res_mode 0, 1 or 2 (2x2-mean down)");
  ConvArgs a{};
  a.xa = xa; a.xb = xb; a.Ca = Ca; a.Cb = Cb;
  a.coef = reinterpret_cast<const Coef*>(coef); a.coef_batch = coef_batch; a.act = act;
  a.resample = resample; a.H = H; a.W = W;
  a.Hs = resample == RS_UP ? H / 2 : H; a.Ws = resample == RS_UP ? W / 2 : W;
  a.wino = wino; a.bias = bias; a.res = res; a.res_mode = res_mode;
  a.out = out; a.Cout = Cout; a.B = B;
  MCEDM_REQUIRE(conv_wino_applicable(a, 9), "op_conv_wino: needs Cout %% 64 == 0, H %% 8 == 0, W %% 16 == 0, Cin %% 8 == 0 and 16-byte aligned inputs / weight table");
  return launch_conv_wino(a, (hipStream_t)stream);
}

// mcedm_op_conv_wino with the fused GroupNorm records of `out` in gsum (4-channel blocks, as a plan's convs write them)
static int op_conv_wino_sums(const float* xa, const float* xb, int Ca, int Cb, const mcedm_coef* coef, int coef_batch, int act,
                             int resample, int H, int W, const float* wino, const float* bias, int bias_batch, const float* res,
                             int res_mode, float* out, float* gsum, int Cout, int B, void* stream) {
  MCEDM_REQUIRE((resample == RS_NONE || resample == RS_UP) && (res_mode == RS_NONE || res_mode == RS_UP || res_mode == RS_DOWN),
                "op_conv_wino_sums: resample must be 0 (none) or 1 (nearest-2x up), res_mode 0, 1 or 2 (2x2-mean down)");
  MCEDM_REQUIRE(gsum, "op_conv_wino_sums: gsum is null");
  ConvArgs a{};
  a.xa = xa; a.xb = xb; a.Ca = Ca; a.Cb = Cb;
  a.coef = reinterpret_cast<const Coef*>(coef); a.coef_batch = coef_batch; a.act = act;
  a.resample = resample; a.H = H; a.W = W;
  a.Hs = resample == RS_UP ? H / 2 : H; a.Ws = resample == RS_UP ? W / 2 : W;
  a.wino = wino; a.bias = bias; a.res = res; a.res_mode = res_mode;
  SumTiles st;
  a.out = out; a.Cout = Cout; a.B = B; a.gsum = gsum; a.gsum_tiles = &st;
  MCEDM_REQUIRE(bias_batch == 0 || (bias && bias_batch >= Cout), "op_conv_wino_sums: bias_batch %d needs a bias of B rows of at least Cout floats", bias_batch);
  a.bias_batch = bias_batch;
  MCEDM_REQUIRE(conv_wino_applicable(a, 9), "op_conv_wino_sums: needs Cout %% 64 == 0, H %% 8 == 0, W %% 16 == 0, Cin %% 8 == 0 and 16-byte aligned inputs / weight table");
  return launch_conv_wino(a, (hipStream_t)stream);
}
extern "C" int mcedm_op_conv_wino_sums(const float* xa, const float* xb, int Ca, int Cb, const mcedm_coef* coef, int coef_batch,
                                       int act, int resample, int H, int W, const float* wino, const float* bias, const float* res,
                                       int res_mode, float* out, float* gsum, int Cout, int B, void* stream) {
  return op_conv_wino_sums(xa, xb, Ca, Cb, coef, coef_batch, act, resample, H, W, wino, bias, 0, res, res_mode, out, gsum, Cout, B, stream);
}
// mcedm_op_conv_wino_sums with a bias row per sample: bias [B][bias_batch]
extern "C" int mcedm_op_conv_wino_sums_bias_batch(const float* xa, const float* xb, int Ca, int Cb, const mcedm_coef* coef,
                                                  int coef_batch, int act, int resample, int H, int W, const float* wino,
                                                  const float* bias, int bias_batch, const float* res, int res_mode, float* out,
                                                  float* gsum, int Cout, int B, void* stream) {
  return op_conv_wino_sums(xa, xb, Ca, Cb, coef, coef_batch, act, resample, H, W, wino, bias, bias_batch, res, res_mode, out, gsum, Cout, B,
                           stream);
}

// The same conv on the SPLIT variant of the Winograd kernel (conv_wino.hpp WinoSplitCfg: images below 32 x 32, Cout % 32 == 0), whatever
// the switch says; gsum: null, or the fused GroupNorm records of `out`.  Bit-identical to mcedm_op_conv_wino(_sums) on a shape both serve.
static int op_conv_wino_split(const char* who, const float* xa, const float* xb, int Ca, int Cb, const mcedm_coef* coef, int coef_batch, int act,
                              int H, int W, const float* wino, const float* bias, const float* res, int res_mode, float* out, float* gsum,
                              int Cout, int B, void* stream) {
  MCEDM_REQUIRE(res_mode == RS_NONE || res_mode == RS_DOWN, "%s: res_mode must be 0 or 2 (2x2-mean down)", who);
  ConvArgs a{};
  a.xa = xa; a.xb = xb; a.Ca = Ca; a.Cb = Cb;
  a.coef = reinterpret_cast<const Coef*>(coef); a.coef_batch = coef_batch; a.act = act;
  a.resample = RS_NONE; a.H = H; a.W = W; a.Hs = H; a.Ws = W;
  a.wino = wino; a.bias = bias; a.res = res; a.res_mode = res_mode;
  SumTiles st;
  a.out = out; a.Cout = Cout; a.B = B; a.gsum = gsum; a.gsum_tiles = gsum ? &st : nullptr;
  MCEDM_REQUIRE(conv_wino_split_applicable(a, 9),
                "%s: needs an image below 32 x 32 with H %% 8 == 0 and W %% 16 == 0, Cout %% 32 == 0, Ca %% 8 == 0, Cin %% 8 == 0 and 16-byte aligned inputs / weight table", who);
  return launch_conv_wino_split(a, (hipStream_t)stream);
}
extern "C" int mcedm_op_conv_wino_split(const float* xa, const float* xb, int Ca, int Cb, const mcedm_coef* coef, int coef_batch, int act,
                                        int H, int W, const float* wino, const float* bias, const float* res, int res_mode, float* out,
                                        int Cout, int B, void* stream) {
  return op_conv_wino_split("op_conv_wino_split", xa, xb, Ca, Cb, coef, coef_batch, act, H, W, wino, bias, res, res_mode, out, nullptr, Cout, B, stream);
}
extern "C" int mcedm_op_conv_wino_split_sums(const float* xa, const float* xb, int Ca, int Cb, const mcedm_coef* coef, int coef_batch, int act,
                                             int H, int W, const float* wino, const float* bias, const float* res, int res_mode, float* out,
                                             float* gsum, int Cout, int B, void* stream) {
  MCEDM_REQUIRE(gsum, "op_conv_wino_split_sums: gsum is null");
  return op_conv_wino_split("op_conv_wino_split_sums", xa, xb, Ca, Cb, coef, coef_batch, act, H, W, wino, bias, res, res_mode, out, gsum, Cout, B, stream);
}

// A 1x1 conv's weights [Cout][Cin] in the MFMA-fragment order of ConvArgs::sk_wfrag (cout_padded(Cout) * ceil8(Cin) floats)
extern "C" int mcedm_op_pack_conv_frag(const float* w, int Cout, int Cin, float* wfrag, void* stream) {
  return launch_pack_conv_frag(w, wfrag, Cout, Cin, (hipStream_t)stream);
}

// conv1 of a decoder block as the plan launches it, through the dispatcher: out = conv3x3(silu(coef(x))) + bias + either the
// residual `res`, or the folded 1x1 projection sk_bias + W_s * cat(sk_xa, sk_xb) (sk_wpk set; sk_wfrag: its fragment-ordered copy,
// which lets the Winograd kernel's SKIP variant serve it), with the fused GroupNorm records in gsum (or null).
extern "C" int mcedm_op_conv_skip(const float* x, int Cin, const mcedm_coef* coef, int act, int H, int W, const float* wpk, const float* wino,
                                  const float* bias, const float* res, const float* sk_xa, const float* sk_xb, int sk_Ca, int sk_Cb,
                                  const float* sk_wpk, const float* sk_wfrag, const float* sk_bias, float* out, float* gsum, int Cout,
                                  int B, void* stream) {
  MCEDM_REQUIRE(x && out && wpk && Cin > 0 && Cout > 0 && B > 0 && H > 0 && W > 0, "op_conv_skip: bad arguments");
  MCEDM_REQUIRE(!(res && sk_wpk), "op_conv_skip: a residual or a folded projection, not both");
  ConvArgs a{};
  a.xa = x; a.Ca = Cin;
  a.coef = reinterpret_cast<const Coef*>(coef); a.coef_batch = 1; a.act = act;
  a.resample = RS_NONE; a.Hs = H; a.Ws = W; a.H = H; a.W = W;
  a.wpk = wpk; a.wino = wino; a.bias = bias; a.res = res; a.res_mode = RS_NONE;
  a.sk_xa = sk_xa; a.sk_xb = sk_xb; a.sk_Ca = sk_Ca; a.sk_Cb = sk_Cb; a.sk_wpk = sk_wpk; a.sk_wfrag = sk_wfrag; a.sk_bias = sk_bias;
  SumTiles st;
  a.out = out; a.Cout = Cout; a.B = B; a.gsum = gsum; a.gsum_tiles = gsum ? &st : nullptr;
  return launch_conv(a, 9, (hipStream_t)stream);
}

// The conv of mcedm_op_conv_bias_batch through the dispatcher (wino: optional Winograd table, as a plan's convs carry one), with what
// the fused GroupNorm chain adds to a launch: the records of `out` (gsum / gsum_rc, the tiling the launcher chose in tiling_out)
// and / or transform rows derived inside the kernel from a producer's records (gn).
static void tiling_to_ints(const SumTiles& t, int* o) { o[0] = t.tiles; o[1] = t.tiles_x; o[2] = t.ph; o[3] = t.pw; o[4] = t.rc; }
static SumTiles tiling_from_ints(const int* t) { return t ? SumTiles{t[0], t[1], t[2], t[3], t[4]} : SumTiles{}; }

static int op_conv_chain(const char* who, const float* xa, const float* xb, int Ca, int Cb, const mcedm_coef* coef, int coef_batch,
                         const GnArgs* gn, int act, int resample, int Hs, int Ws, int H, int W, const float* wpk, const float* wino,
                         const float* bias_pk, int bias_batch, const float* res, int res_mode, float* out, int Cout, int B, int k,
                         float* gsum, int gsum_rc, int* tiling_out, void* stream) {
  MCEDM_REQUIRE(k == 1 || k == 3, "%s: k must be 1 or 3", who);
  MCEDM_REQUIRE(resample >= 0 && resample <= 3 && res_mode >= 0 && res_mode <= 2, "%s: bad resample mode", who);
  MCEDM_REQUIRE(bias_batch >= 0, "%s: bias_batch %d < 0", who, bias_batch);
  ConvArgs a{};
  a.xa = xa; a.xb = xb; a.Ca = Ca; a.Cb = Cb;
  a.coef = reinterpret_cast<const Coef*>(coef); a.coef_batch = coef_batch; a.act = act;
  a.resample = resample; a.Hs = Hs; a.Ws = Ws; a.H = H; a.W = W;
  a.wpk = wpk; a.wino = wino; a.bias = bias_pk; a.res = res; a.res_mode = res_mode;
  a.out = out; a.Cout = Cout; a.B = B; a.bias_batch = bias_batch;
  SumTiles st;
  if (gsum) { a.gsum = gsum; a.gsum_rc = gsum_rc; a.gsum_tiles = &st; }
  if (gn) { a.gn = *gn; a.gn_on = 1; a.coef = nullptr; a.coef_batch = 1; }
  const int rc = launch_conv(a, k * k, (hipStream_t)stream);
  if (rc) return rc;
  if (gsum) {
    MCEDM_REQUIRE(st.tiles > 0 && st.rc == (gsum_rc == 2 ? 2 : 4), "%s: the launcher wrote no tiling, or records of %d channels where %d were asked for",
                  who, st.rc, gsum_rc == 2 ? 2 : 4);
    tiling_to_ints(st, tiling_out);
  }
  return MCEDM_OK;
}

extern "C" int mcedm_op_conv_sums(const float* xa, const float* xb, int Ca, int Cb, const mcedm_coef* coef, int coef_batch, int act,
                                  int resample, int Hs, int Ws, int H, int W, const float* wpk, const float* wino, const float* bias_pk,
                                  int bias_batch, const float* res, int res_mode, float* out, int Cout, int B, int k, float* gsum,
                                  int gsum_rc, int* tiling_out, void* stream) {
  MCEDM_REQUIRE(gsum && tiling_out, "op_conv_sums: gsum / tiling_out is null");
  MCEDM_REQUIRE(gsum_rc == 0 || gsum_rc == 2 || gsum_rc == 4, "op_conv_sums: gsum_rc = %d, records hold 4 (0 / 4) or 2 channels", gsum_rc);
  // a partial record's element count is not the rc * h * w the consumers assume (sum_tile_count); no plan asks for one
  MCEDM_REQUIRE(Cout > 0 && Cout % (gsum_rc == 2 ? 2 : 4) == 0, "op_conv_sums: Cout = %d is not a whole number of %d-channel records", Cout,
                gsum_rc == 2 ? 2 : 4);
  return op_conv_chain("op_conv_sums", xa, xb, Ca, Cb, coef, coef_batch, nullptr, act, resample, Hs, Ws, H, W, wpk, wino, bias_pk, bias_batch,
                       res, res_mode, out, Cout, B, k, gsum, gsum_rc, tiling_out, stream);
}

// The GnArgs of a consumer of records: cat(a, b) [B, Ca + Cb, H, W] described by its producers' tables alone (no tensor pointers)
static int op_gn_from_records(const char* who, GnArgs& g, const float* suma, const float* sumb, const int* tiling_a, const int* tiling_b,
                              int Ca, int Cb, int B, int H, int W, int groups, const float* gamma, const float* beta, const float* film,
                              int film_batch, int film_stride, float eps) {
  MCEDM_REQUIRE(suma && tiling_a && gamma && beta, "%s: null pointer", who);
  MCEDM_REQUIRE(B > 0 && H > 0 && W > 0 && Ca > 0 && Cb >= 0 && groups > 0, "%s: bad shape", who);
  MCEDM_REQUIRE(Cb == 0 || (sumb && tiling_b), "%s: Cb = %d without the second table", who, Cb);
  MCEDM_REQUIRE((Ca + Cb) % groups == 0, "%s: C=%d not divisible by groups=%d", who, Ca + Cb, groups);
  g = GnArgs{nullptr, nullptr, Ca, Cb, H * W, B, groups, gamma, beta, film, film_batch, film_stride, eps, nullptr, nullptr, suma,
             Cb ? sumb : nullptr, tiling_from_ints(tiling_a), Cb ? tiling_from_ints(tiling_b) : SumTiles{}, W};
  for (const SumTiles* t : {&g.ta, &g.tb}) {
    if (t == &g.tb && !Cb) break;
    MCEDM_REQUIRE(t->tiles > 0 && t->tiles_x > 0 && t->ph > 0 && t->pw > 0 && t->tiles_x == ceil_div(W, t->pw) &&
                      t->tiles == t->tiles_x * ceil_div(H, t->ph),
                  "%s: tiling (%d tiles, %d across, %d x %d pixels) does not cover a %d x %d image", who, t->tiles, t->tiles_x, t->ph, t->pw, H, W);
  }
  // never the pass over the tensor that launch_gn_coef_from_sums falls back to: the caller has to know which kernel ran
  MCEDM_REQUIRE(gn_sums_usable(g), "%s: records of %d | %d channels (%d / %d per record) do not tile %d groups", who, Ca, Cb, g.ta.rc,
                Cb ? g.tb.rc : g.ta.rc, groups);
  return MCEDM_OK;
}

// gn_coef_from_sums_kernel on its own: the transform table (+ statistics) of GroupNorm(groups) (+ FiLM) from records alone
extern "C" int mcedm_op_gn_coef_from_sums(const float* suma, const float* sumb, const int* tiling_a, const int* tiling_b, int Ca, int Cb,
                                          int B, int H, int W, int groups, const float* gamma, const float* beta, const float* film,
                                          int film_batch, int film_stride, float eps, mcedm_coef* coef_out, float* stats_out,
                                          void* stream) {
  MCEDM_REQUIRE(coef_out, "op_gn_coef_from_sums: null pointer");
  GnArgs g;
  const int rc = op_gn_from_records("op_gn_coef_from_sums", g, suma, sumb, tiling_a, tiling_b, Ca, Cb, B, H, W, groups, gamma, beta, film,
                                    film_batch, film_stride, eps);
  if (rc) return rc;
  g.coef = reinterpret_cast<Coef*>(coef_out); g.stats = stats_out;
  return launch_gn_coef_from_sums(g, (hipStream_t)stream);
}

// A conv whose transform rows come from records inside the kernel (ConvArgs::gn_on, stage_coef_rows): the records describe the
// SOURCE cat(xa, xb) [B, Ca + Cb, Hs, Ws]
extern "C" int mcedm_op_conv_gn(const float* xa, const float* xb, int Ca, int Cb, const float* suma, const float* sumb, const int* tiling_a,
                                const int* tiling_b, int groups, const float* gamma, const float* beta, const float* film, int film_batch,
                                int film_stride, float eps, int act, int resample, int Hs, int Ws, int H, int W, const float* wpk,
                                const float* wino, const float* bias_pk, const float* res, int res_mode, float* out, int Cout, int B, int k,
                                void* stream) {
  GnArgs g;
  const int rc = op_gn_from_records("op_conv_gn", g, suma, sumb, tiling_a, tiling_b, Ca, Cb, B, Hs, Ws, groups, gamma, beta, film, film_batch,
                                    film_stride, eps);
  if (rc) return rc;
  return op_conv_chain("op_conv_gn", xa, xb, Ca, Cb, nullptr, 1, &g, act, resample, Hs, Ws, H, W, wpk, wino, bias_pk, 0, res, res_mode, out,
                       Cout, B, k, nullptr, 0, nullptr, stream);
}

// freqs[k] = (1/10000)^(k/half) exactly as the plan packs them (adm_blocks.py:193-196, endpoint=False)
__global__ void op_freqs_kernel(float* f, int half) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k < half) f[k] = (float)pow((double)(1.0f / 10000.0f), (double)((float)k / (float)half));
}

extern "C" int mcedm_op_embedding(const float* labels, int n, int ch, const float* w0, const float* b0, const float* w1,
                                  const float* b1, const float* waff, const float* baff, int rows, float* freqs_scratch,
                                  float* emb_out, float* film_out, void* stream) {
  MCEDM_REQUIRE(labels && w0 && b0 && w1 && b1 && waff && baff && freqs_scratch && film_out, "op_embedding: null pointer");
  MCEDM_REQUIRE(n > 0 && ch > 0 && ch % 2 == 0 && rows > 0, "op_embedding: bad shape n=%d ch=%d rows=%d", n, ch, rows);
  hipLaunchKernelGGL(op_freqs_kernel, dim3(ceil_div(ch / 2, 64)), dim3(64), 0, (hipStream_t)stream, freqs_scratch, ch / 2);
  MCEDM_LAUNCH_CHECK("op_freqs_kernel");
  EmbArgs e{labels, n, ch, freqs_scratch, w0, b0, w1, b1, waff, baff, rows, emb_out, film_out};
  return launch_embedding(e, (hipStream_t)stream);
}

extern "C" int mcedm_op_attention(const float* qkv, float* out, int B, int heads, int T, void* stream) {
  MCEDM_REQUIRE(qkv && out, "op_attention: null pointer");
  return launch_attention(qkv, out, B, heads, T, (hipStream_t)stream);
}

// The fused 8 x 8 x 64 attention block (attn_fused.hip) on its own, whatever MCEDM_ATTN_FUSED / mcedm_op_set_attn_fused say
extern "C" int mcedm_op_attn_block64(const float* y, const float* gamma, const float* beta, float eps, const float* wq_pk,
                                     const float* bq_pk, const float* wp_pk, const float* bp_pk, float* z, float* gsum, int B,
                                     void* stream) {
  MCEDM_REQUIRE(y && z && gamma && beta && wq_pk && bq_pk && wp_pk && bp_pk, "op_attn_block64: null pointer");
  MCEDM_REQUIRE(B > 0, "op_attn_block64: B = %d", B);
  return launch_attn_block64(y, z, gamma, beta, eps, 16, wq_pk, bq_pk, wp_pk, bp_pk, gsum, nullptr, B, (hipStream_t)stream);
}

extern "C" int mcedm_op_set_conv_tile(int mt, int ph, int pw) {
  set_conv_tile_override(mt, ph, pw);
  return MCEDM_OK;
}

extern "C" size_t mcedm_op_wgrad_scratch_floats(int Cout, int Cin, int k, int B, int H, int W) {
  if (Cout <= 0 || Cin <= 0 || (k != 1 && k != 3) || B <= 0 || H <= 0 || W <= 0) return 0;
  return align_up(wgrad_scratch_floats(Cout, Cin, k * k), 64) + (size_t)B * Cin * H * W;
}

extern "C" int mcedm_op_conv_wgrad(const float* dy, const float* xa, const float* xb, int Ca, int Cb,
                                   const mcedm_coef* coef, int coef_batch, int act, int resample, int Hs, int Ws, int H,
                                   int W, int Cout, int B, int k, int qkv_heads, float* scratch, float* dw, float* db,
                                   void* stream) {
  MCEDM_REQUIRE(k == 1 || k == 3, "op_conv_wgrad: k must be 1 or 3");
  MCEDM_REQUIRE(dy && scratch && dw, "op_conv_wgrad: null pointer");
  WgradArgs a{dy, xa, xb, Ca, Cb, reinterpret_cast<const Coef*>(coef), coef_batch, act, resample, Hs, Ws, H, W, Cout, B,
              scratch, nullptr};
  float* act_tmp = scratch + align_up(wgrad_scratch_floats(Cout, Ca + Cb, k * k), 64);
  return launch_wgrad(a, k * k, dw, db, qkv_heads, act_tmp, (hipStream_t)stream);
}

static int op_gn_bwd_impl(const float* dact, int resample, const float* xa, const float* xb, int Ca, int Cb, int Hs,
                               int Ws, int B, const mcedm_coef* coef, const float* stats, const float* gamma,
                               const float* beta, const float* film, int film_batch, int film_stride, int act,
                               float* dxa, float* dxb, int accumulate, const float* add, int add_mode, float* ab,
                               float* dgamma, float* dbeta, float* dfilm, int dfilm_stride, unsigned* sync, void* stream) {
  MCEDM_REQUIRE(dact && xa && coef && stats && gamma && beta && dxa && ab && dgamma && dbeta, "op_gn_bwd: null pointer");
  const int C = Ca + Cb;
  MCEDM_REQUIRE(C >= 4, "op_gn_bwd: C < 4");
  GnBwdArgs a{dact, resample, xa, xb, Ca, Cb, Hs, Ws, B, C / 4 < 32 ? C / 4 : 32, reinterpret_cast<const Coef*>(coef),
              stats, gamma, film, film_batch, film_stride, act, dxa, dxb, accumulate, add, add_mode, C, ab};
  a.sync = sync;
  int rc = launch_gn_bwd(a, (hipStream_t)stream);
  if (rc) return rc;
  return launch_gn_param_grads(ab, gamma, beta, film, film_batch, film_stride, B, C, dgamma, dbeta, dfilm, dfilm_stride,
                               (hipStream_t)stream);
}

extern "C" int mcedm_op_gn_bwd(const float* dact, int resample, const float* xa, const float* xb, int Ca, int Cb, int Hs,
                               int Ws, int B, const mcedm_coef* coef, const float* stats, const float* gamma,
                               const float* beta, const float* film, int film_batch, int film_stride, int act,
                               float* dxa, float* dxb, int accumulate, const float* add, int add_mode, float* ab,
                               float* dgamma, float* dbeta, float* dfilm, int dfilm_stride, void* stream) {
  return op_gn_bwd_impl(dact, resample, xa, xb, Ca, Cb, Hs, Ws, B, coef, stats, gamma, beta, film, film_batch, film_stride, act, dxa, dxb,
                        accumulate, add, add_mode, ab, dgamma, dbeta, dfilm, dfilm_stride, nullptr, stream);
}

extern "C" int mcedm_op_gn_bwd_sync(const float* dact, int resample, const float* xa, const float* xb, int Ca, int Cb, int Hs,
                                    int Ws, int B, const mcedm_coef* coef, const float* stats, const float* gamma,
                                    const float* beta, const float* film, int film_batch, int film_stride, int act,
                                    float* dxa, float* dxb, int accumulate, const float* add, int add_mode, float* ab,
                                    float* dgamma, float* dbeta, float* dfilm, int dfilm_stride, unsigned int* sync, void* stream) {
  return op_gn_bwd_impl(dact, resample, xa, xb, Ca, Cb, Hs, Ws, B, coef, stats, gamma, beta, film, film_batch, film_stride, act, dxa, dxb,
                        accumulate, add, add_mode, ab, dgamma, dbeta, dfilm, dfilm_stride, sync, stream);
}

extern "C" int mcedm_op_attention_bwd(const float* qkv, const float* a, const float* da, float* dqkv, float* lse_scratch,
                                      int B, int heads, int T, void* stream) {
  return launch_attention_bwd(qkv, a, da, dqkv, lse_scratch, B, heads, T, (hipStream_t)stream);
}

// the process-wide level of the kernel switches (switches.hpp): any integer, < 0 = not set
static int set_switch(KernelVariant which, int value) { set_kernel_switch(which, value); return MCEDM_OK; }
extern "C" int mcedm_op_set_conv8(int enable) { return set_switch(KV_CONV8, enable); }
extern "C" int mcedm_op_set_conv_wino(int enable) { return set_switch(KV_CONV_WINO, enable); }
extern "C" int mcedm_op_set_conv_wino1(int enable) { return set_switch(KV_CONV_WINO1, enable); }
extern "C" int mcedm_op_set_conv_wino_fold(int enable) { return set_switch(KV_CONV_WINO_FOLD, enable); }
extern "C" int mcedm_op_set_conv_wino_upz(int enable) { return set_switch(KV_CONV_WINO_UPZ, enable); }
extern "C" int mcedm_op_set_conv_wino_split(int enable) { return set_switch(KV_CONV_WINO_SPLIT, enable); }
extern "C" int mcedm_op_set_conv1x1_reg(int enable) { return set_switch(KV_CONV1X1_REG, enable); }
extern "C" int mcedm_op_set_wgrad_wino(int enable) { return set_switch(KV_WGRAD_WINO, enable); }
extern "C" int mcedm_op_set_conv_resident(int enable) { return set_switch(KV_CONV_RESIDENT, enable); }
extern "C" int mcedm_op_set_attn_fused(int enable) { return set_switch(KV_ATTN_FUSED, enable); }

extern "C" int mcedm_op_set_conv_debug(unsigned long long* buf) {
  set_conv_debug(buf);
  return MCEDM_OK;
}

// one step of the conditional DDIM sampler (edm.hip: ddim_cond_step_kernel) on caller-owned tensors
static int op_ddim_cond_step(const float* xt, const float* F, const float* Fu, const float* noise, const uint64_t* rng_seed,
                             uint64_t draw, double w, float s0, float s1, float sa_next, float c1, float c2, float* xt_next,
                             float* condp, float* condp_u, int cond_channels, int plan_cond_channels, int B, int C, int H, int W,
                             float* xs, int T_xs, int t_xs, float* x0s, int T_x0, int t_x0, void* stream, const float* dx = nullptr,
                             float gw = 0.f) {
  MCEDM_REQUIRE(xt && F && xt_next, "op_ddim_cond_step: null pointer");
  MCEDM_REQUIRE(!(noise && rng_seed), "op_ddim_cond_step: noise and rng_seed are both given (at most one of them)");
  MCEDM_REQUIRE(!dx || C == 1, "op_ddim_cond_step: dx [B, 1, H, W] goes with C == 1 (got C = %d)", C);
  MCEDM_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0, "op_ddim_cond_step: empty shape");
  MCEDM_REQUIRE(!condp_u || condp, "op_ddim_cond_step: the twin goes with cond'");
  MCEDM_REQUIRE(!condp || (cond_channels >= 0 && cond_channels + C <= plan_cond_channels),
                "op_ddim_cond_step: channels [%d, %d) outside cond' (%d channels)", cond_channels, cond_channels + C, plan_cond_channels);
  MCEDM_REQUIRE((!xs || (t_xs >= 0 && t_xs < T_xs)) && (!x0s || (t_x0 >= 0 && t_x0 < T_x0)), "op_ddim_cond_step: slot outside the trajectory");
  DdimCondStep k{};
  k.xt = xt; k.F = F; k.Fu = Fu; k.noise = noise;
  k.seed = reinterpret_cast<const unsigned long long*>(rng_seed); k.draw = draw;
  k.w1 = (float)(w + 1.0); k.w = (float)w; k.s0 = s0; k.s1 = s1; k.sa = sa_next; k.c1 = c1; k.c2 = c2;
  k.xt_next = xt_next; k.sc = condp; k.sc_u = condp_u;
  k.C = C; k.Cp = plan_cond_channels; k.sc_off = cond_channels; k.hw = (size_t)H * W; k.n = (size_t)B * C * k.hw;
  k.xs = xs; k.x0s = x0s; k.T_xs = T_xs; k.t_xs = t_xs; k.T_x0 = T_x0; k.t_x0 = t_x0;
  k.dxg = dx; k.gw = dx ? gw : 0.f;
  return launch_ddim_cond_step(k, (hipStream_t)stream);
}
extern "C" int mcedm_op_ddim_cond_step(const float* xt, const float* F, const float* Fu, const float* noise, double w, float s0,
                                       float s1, float sa_next, float c1, float c2, float* xt_next, float* condp, float* condp_u,
                                       int cond_channels, int plan_cond_channels, int B, int C, int H, int W, float* xs,
                                       int T_xs, int t_xs, float* x0s, int T_x0, int t_x0, void* stream) {
  return op_ddim_cond_step(xt, F, Fu, noise, nullptr, 0, w, s0, s1, sa_next, c1, c2, xt_next, condp, condp_u, cond_channels,
                           plan_cond_channels, B, C, H, W, xs, T_xs, t_xs, x0s, T_x0, t_x0, stream);
}
// the same step with its uniform noise generated in the kernel: draw `draw` of mcedm_uniform_fill keyed by *rng_seed
extern "C" int mcedm_op_ddim_cond_step_rng(const float* xt, const float* F, const float* Fu, const uint64_t* rng_seed, uint64_t draw,
                                           double w, float s0, float s1, float sa_next, float c1, float c2, float* xt_next,
                                           float* condp, float* condp_u, int cond_channels, int plan_cond_channels, int B, int C,
                                           int H, int W, float* xs, int T_xs, int t_xs, float* x0s, int T_x0, int t_x0,
                                           void* stream) {
  MCEDM_REQUIRE(rng_seed != nullptr, "op_ddim_cond_step_rng: rng_seed (a 64-bit seed in device memory) is null");
  return op_ddim_cond_step(xt, F, Fu, nullptr, rng_seed, draw, w, s0, s1, sa_next, c1, c2, xt_next, condp, condp_u, cond_channels,
                           plan_cond_channels, B, C, H, W, xs, T_xs, t_xs, x0s, T_x0, t_x0, stream);
}
// both forms in one signature, with the PDE-guidance term et -= gw * dx (dx [B, 1, H, W], C == 1; NULL: the step above)
extern "C" int mcedm_op_ddim_cond_step_guided(const float* xt, const float* F, const float* Fu, const float* noise,
                                              const uint64_t* rng_seed, uint64_t draw, const float* dx, float gw, double w, float s0,
                                              float s1, float sa_next, float c1, float c2, float* xt_next, float* condp, float* condp_u,
                                              int cond_channels, int plan_cond_channels, int B, int C, int H, int W, float* xs,
                                              int T_xs, int t_xs, float* x0s, int T_x0, int t_x0, void* stream) {
  return op_ddim_cond_step(xt, F, Fu, noise, rng_seed, draw, w, s0, s1, sa_next, c1, c2, xt_next, condp, condp_u, cond_channels,
                           plan_cond_channels, B, C, H, W, xs, T_xs, t_xs, x0s, T_x0, t_x0, stream, dx, gw);
}

// the two kernels of the training step's dropout (edm.hip) on caller-owned tensors
extern "C" int mcedm_op_dropout_act(const float* h, const mcedm_coef* coef, int coef_batch, float* out, int B, int C, int H, int W,
                                    double p, const uint64_t* rng_seed, uint64_t draw, void* stream) {
  return launch_dropout_act(h, reinterpret_cast<const Coef*>(coef), coef_batch, out, B, C, H, W, p,
                            reinterpret_cast<const unsigned long long*>(rng_seed), draw, (hipStream_t)stream);
}
extern "C" int mcedm_op_dropout_scale(float* g, int B, int C, int H, int W, double p, const uint64_t* rng_seed, uint64_t draw,
                                      void* stream) {
  MCEDM_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0, "op_dropout_scale: empty shape");
  return launch_dropout_scale(g, (size_t)B * C * H * W, p, reinterpret_cast<const unsigned long long*>(rng_seed), draw,
                              (hipStream_t)stream);
}
