// conv_wino.hpp -- constants and LDS layouts shared by the two Winograd F(2x2, 3x3) kernels (conv_wino.hip: eight waves per
// workgroup, two per SIMD; conv_wino1.hip: four waves, one per SIMD with all sixteen positions).  Device code only.
#pragma once
#include "conv_tile.hpp"

namespace mcedm {

constexpr int WPH = 8, WPW = 16;                 // output pixels per workgroup
constexpr int WTX = WPW / 2, WTY = WPH / 2;      // 2x2 patches: 8 x 4 = 32 = one MFMA N block
constexpr int WKC = 8;                           // input channels per chunk
static_assert(WTX * WTY == 32, "one MFMA N block of patches per workgroup");
// MB = 32-channel output blocks per workgroup: 4 (128 channels, 512 threads, one workgroup per CU, two chunks per stage) or
// 2 (64 channels -- the ch = 64 networks --, 256 threads, two workgroups per CU, one chunk per stage so that both fit the LDS)
template <int MB_>
struct WinoCfg {
  static constexpr int MB = MB_, NT = 128 * MB_, NW = 2 * MB_, MT = 32 * MB_;
  static constexpr int SC = MB_ == 4 ? 2 : 1;          // chunks per stage of the K loop (one barrier per stage)
  static constexpr int CPW = WKC / NW;                  // channels of a chunk that one wave stages: 1 or 2
  static constexpr int TI = 4 / MB_;                    // patch rows (of the four) per thread in the input transform
  static constexpr int VBUF = SC * 16 * 288, RBUF = SC * WKC * 196;      // floats per stage (VPOS, RPLANE below)
  static constexpr int LDS_ROWS_OFF = 2 * VBUF + 2 * RBUF;              // transform rows start here (floats; 16-byte aligned)
  static constexpr int XCH_FLOATS = NW * 16 * 64;                       // epilogue exchange: one round of 16 registers x 64 lanes per wave
  static constexpr int RED_FLOATS = 2 * (MT / 2) * 3 + MT;              // statistics records of the two halves (pairs at most) + the bias row
  static constexpr bool SKIP = false;                                   // see WinoSkipCfg
  static constexpr bool SPLIT = false;                                  // see WinoSplitCfg
  static_assert(MB_ == 4 || MB_ == 2, "128 or 64 output channels per workgroup");
  static_assert(LDS_ROWS_OFF % 4 == 0, "LDS layout");
};
// The SPLIT variant, for images below the other variants' minimum size (16 x 16: at B = 32 a 128-channel workgroup per pixel tile
// leaves three quarters of the chip idle): a workgroup is ONE 32-channel output block x one pixel tile x all sixteen positions,
// and the POSITIONS are split over the eight waves -- wave w owns positions 2 w, 2 w + 1 (xi = w >> 1, nu = 2 (w & 1) + {0, 1}): two
// accumulator blocks, eight MFMAs per chunk.  The input path is WinoCfg<4>'s, instruction for instruction (512 threads, two chunks
// per stage, wave w stages channel w of a chunk, thread = (channel, patch, row half) in the transform); the epilogue passes all
// sixteen blocks through LDS (64 KB over the drained V buffers) and evaluates the output transform in the expression tree of the
// other variants -- over nu, then over xi, keep + the partner's send, residual -- on their lane layout (wave = row half x
// four-register group), so outputs and GroupNorm records carry the bits of WinoCfg<4> / WinoCfg<2> on the same shape.
// A configuration class of its own: an instantiation and a profiler name of its own, the other variants keep theirs.
struct WinoSplitCfg : WinoCfg<4> {
  static constexpr int MT = 32;                                         // output channels per workgroup
  static constexpr int XCH_FLOATS = 0;                                  // no exchange area: the accumulator dump aliases the V buffers
  static constexpr int RED_FLOATS = 2 * (MT / 2) * 3 + MT;
  static constexpr int DUMP_FLOATS = 16 * 16 * 64;                      // sixteen blocks of 16 registers x 64 lanes
  static constexpr bool SPLIT = true;
  static_assert(DUMP_FLOATS <= 2 * VBUF, "the accumulator dump fits the two V buffers");
};
// The SKIP variant (ConvArgs::sk_wfrag): the epilogue COMPUTES the residual -- the decoder block's 1x1 skip projection of
// cat(sk_xa, sk_xb), 32 channels x 64 pixels per wave -- on the matrix pipe instead of loading it.  A configuration class of its
// own, so that it is an instantiation of its own and the other variants keep their code and their names.
//   raw input: stages of SKS channels x the tile's 8 x 16 pixels, one 16-byte load per thread, through two LDS buffers in the
//   B-operand order [row half][patch][channel parity][k-step][pixel of the pair]; patches SKPITCH = 36 floats apart (= 4 mod 32:
//   the sixteen lanes of a ds_read_b128 group cover the 64 banks once)
template <int MB_>
struct WinoSkipCfg : WinoCfg<MB_> {
  static constexpr bool SKIP = true;
  static constexpr int SKS = 16, SKPITCH = 36, SKBUF = 64 * SKPITCH;
  static constexpr int SK_FLOATS = WinoCfg<MB_>::MT + 2 * SKBUF;        // the projection's bias row, two stage buffers
  static_assert(MB_ == 4, "the fold is built for the 128-channel workgroup (512 threads = 16 channels x 32 quads per stage)");
};
// The zero-position variant of the UP-SAMPLING kernel (UP == true only; WinoUp below).  The input is the nearest 2x up-sampling of the source and
// tiles and patches start on even pixels, so the rows (and likewise the columns) of every 4 x 4 input patch are (a, b, b, c) in source
// pixels -- zero padding is source row / column -1 or Hs / Ws, rows 1 and 2 are always both inside the image.  Under B^T the patch
// gives xi = 0: a - b, xi = 1: b + b, xi = 2: b - b = +0, xi = 3: b - c, and the same along nu (the negated nu = 2 column is
// c1 + (-1) c2 = +0): at the SEVEN positions with xi = 2 or nu = 2 V is exactly +0 for every channel, patch and sample.  Their
// products are +-0, an accumulator that starts at +0 stays +0 under round-to-nearest, and the bias sits at (1, 1): the variant does
// nothing for them (no weight load, no B-fragment read, no MFMA; nu = 2 is not written to the V tile either) and the epilogue
// meets the same +0 blocks as before.  PRECONDITION: finite transformed weights (0 * Inf would have been NaN).
// Blocks are ordered by liveness: hf = 1 keeps xi = 3 in acc[0..3] (xi = 2, dead, in acc[4..7]), so that blocks 0, 1, 3 are what
// both halves run and blocks 4, 5, 7 (xi = 1) what only the hf = 0 waves run: 6 + 3 of 16 positions per SIMD.
// SRC: the raw tile is staged at SOURCE resolution -- the 6 x 10 source pixels (4 x 8 plus a halo of one) under the tile's 10 x 18
// patch: ONE dword load, one (x - mean) * scale + offset -> SiLU evaluation, one mask and one LDS store per lane and channel instead
// of three -- and the transform reads source rows ty + {0, 1, 2} and columns tx + {0, 1, 2} of patch (ty, tx): patch row r is source
// row (r + 1) >> 1 of the staged patch.  It evaluates the same expressions on the same values (Y - X, X + s Z down the rows;
// c0 - c2, c1 + c2, c1 - c3 along the columns), hence the same bits.  SRC = false keeps the element-by-element staging of the
// sixteen-position kernel (the positions alone: switch value 2, kept for A/B runs).
// A TAG behind the kernel's own template arguments -- conv_wino_kernel<WinoCfg<MB>, true, true, WinoUp<SRC>> --: an instantiation and a
// profiler name of its own (KV_CONV_WINO_UPZ picks it) that still reads as the up-sampling kernel of WinoCfg<MB>; without a tag (every
// other instantiation) the kernel and its name are what they were.
template <bool SRC>
struct WinoUp {};
template <class... Tag>
struct WinoUpTraits { static constexpr bool UPZ = false, UPS = false, BROWS = false, LOOP1 = false; static_assert(sizeof...(Tag) == 0, "one tag at most: WinoUp<SRC> or WinoBiasRows"); };
template <bool SRC>
struct WinoUpTraits<WinoUp<SRC>> { static constexpr bool UPZ = true, UPS = SRC, BROWS = false, LOOP1 = false; };
// WinoBiasRows: the un-resampled, activated kernel with a bias row per sample (ConvArgs::bias_batch).  An instantiation of its own:
// the kernel sits at 256 registers, and reading one more argument in the shared prologue cost the 128-channel form its schedule
// (2 % of its time) although no resource count moved; without the tag the kernel is what it was, instruction for instruction.
struct WinoBiasRows {};
template <>
struct WinoUpTraits<WinoBiasRows> { static constexpr bool UPZ = false, UPS = false, BROWS = true, LOOP1 = false; };
// WinoLoop1, in FRONT of the other tag: the K loop with one stage per trip and run-time addresses -- the LDS buffer parity added to a
// lane index in front of every group of accesses, the weights through a 64-bit pointer per lane.  Without it (the default, every
// launch of the benchmark workloads) a trip is TWO stages with the parity a compile-time constant: every LDS address is a per-lane
// register computed once per workgroup plus an immediate offset, and the weights go through one buffer descriptor with the chunk in
// the scalar offset -- no address arithmetic between the MFMAs.  That form ends a tile only behind the
// second stage of a trip (the epilogue exists once in the loop), so the launcher keeps WinoLoop1 for the shapes with an odd
// number of stages per tile and for a Winograd table beyond a descriptor's 4 GiB range.  Same operations in the same order: same bits.
struct WinoLoop1 {};
template <class... Tag>
struct WinoUpTraits<WinoLoop1, Tag...> : WinoUpTraits<Tag...> { static constexpr bool LOOP1 = true; };
constexpr int UROWS = WPH / 2 + 2, UCOLS = WPW / 2 + 2;   // source patch of a tile: 6 x 10
constexpr int UPLANE = 68;                       // floats between its channels (60 used; lanes 60 .. 63 store into the pad); = 4 mod 32: the
                                                 // transform's dword reads (eight channels x four patch columns per 32 lanes) cover the 32 banks once
static_assert(UPLANE >= 64 && UPLANE % 32 == 4 && UPLANE <= 196, "LDS layout");
constexpr int RROWS = WPH + 2, RPITCH = WPW + 2; // raw tile with halo: 10 x 18
constexpr int RPLANE = 196;                      // floats between channels of the raw tile (180 used); = 4 mod 32: hipcc merges the transform's two
                                                 // adjacent 8-byte reads into ds_read2_b64, which banks at dword mod 32 over 16-lane groups = eight
                                                 // channels x two patch columns x two dwords: channels 4 banks apart cover the 32 banks once
constexpr int RSUB = (RROWS * RPITCH + 63) / 64; // raw elements per lane and channel: 3
constexpr int WINO_IL_K = 5;                     // side-work instructions the K loop's recipe admits behind each MFMA
// V tile of one (chunk, position): [k parity h][patch 32][k-step 4]; the h = 1 block starts at float 144 = 16 mod 32: the
// transform's dword writes bank at dword mod 32 per 32-lane group (four patch columns x eight channels: 4 ttx + (k >> 1) + 16 (k & 1)
// covers the 32 banks once); the 16-byte B-fragment reads (dword mod 64, 16-lane groups inside one h half) only need it 16-byte
// aligned.  (160 and RPLANE 208, the first layout, were 2-way on those writes and 4-way on the transform's reads:
// SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE = 0.48, profiles/r3_s128_mfma_lds_counters.json.)
constexpr int VH1 = 144, VPOS = 288;
static_assert(RPLANE % 32 == 4 && VH1 % 32 == 16 && VH1 >= 128 && VPOS >= VH1 + 128 && RPLANE >= RROWS * RPITCH && RPLANE % 2 == 0 && VPOS % 4 == 0 && VH1 % 4 == 0, "LDS layout");



// conv_wino1.hip: the 128-channel shape with ONE wave per SIMD (see there); -1: not served (shape / switch), else the launch status
int try_launch_conv_wino1(const ConvArgs& a, hipStream_t stream);
// tiles per persistent workgroup (a divisor of the tiles per image; conv_wino.hip)
int wino_tiles_per_wg(long long total, int tiles_img, int slots);
// MCEDM_WINO_PER: force the tiles per workgroup of both kernels (A/B runs; must divide the tiles per image)
inline int wino_per_env() { static const int v = env_int("MCEDM_WINO_PER", 0); return v; }

}  // namespace mcedm
