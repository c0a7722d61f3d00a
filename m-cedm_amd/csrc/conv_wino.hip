// conv_wino.hip -- the un-resampled 3x3 convolution of the 128-channel levels in Winograd F(2x2, 3x3) form.
//
// Why: on gfx950 the fp32 matrix rate (v_mfma_f32_32x32x2_f32, 157.3 TFLOP/s dense) bounds conv_mfma_kernel, whose K loop
// already runs at 97 % of it.  The only thing left is to issue fewer MFMAs: F(2x2, 3x3) computes a
// 2 x 2 output patch from a 4 x 4 input patch with 16 multiplies per (cin, cout) instead of 36 -- 2.25x less matrix work --
// at the price of a 4x larger accumulator footprint (16 Winograd-domain values per 4 outputs) and of input / output
// transforms in vector instructions (which are paid in matrix time on this chip).
//
//   y = A^T [ sum_cin (G g G^T) o (B^T d B) ] A        (Lavin & Gray 2016; B, G, A below)
//
// Mapping to one CU (one 512-thread workgroup = 8 waves, 2 per SIMD):
//   * workgroup tile = 128 output channels x (8 x 16 pixels = 32 patches) x 16 Winograd positions = 64 accumulator blocks
//     of 32 x 32 = half of the CU's register file.  Wave (mb, hf) owns output channels 32 mb .. + 31 and the eight
//     positions (xi, nu) with xi in {2 hf, 2 hf + 1}: 128 accumulator registers.
//   * K loop over chunks of 8 input channels.  Per chunk and wave: 8 positions x 4 k-steps = 32 MFMAs; the A operand
//     (transformed weights U = G g G^T, packed per (chunk, 32-channel block, position, lane) so that a lane's four k-steps
//     are one 16-byte load) comes straight from L2 into registers, one chunk ahead -- no weight slab in LDS; the B operand
//     (transformed input V = B^T d B, LDS layout [position][patch][k parity][k-step]) is one ds_read_b128 per position.
//   * input path per chunk: wave w loads channel w of the chunk (10 x 18 raw patch incl. halo, 3 elements per lane), applies
//     the fused (x - mean) * scale + offset -> SiLU transform and writes the raw tile to LDS; one stage later every thread
//     turns (channel k, patch t, row half) of it into 8 Winograd-domain values (6 ds_read_b64, 16 adds, 8 ds_write_b32).
//     Both LDS stages are double-buffered, a stage is two chunks, ONE barrier per stage, and all of this side work is
//     issued in slices between the MFMAs of the same wave (see the K loop).
//     A trip of the loop is TWO stages, buffer parity 0 and 1 as compile-time constants: every LDS address is a per-lane register
//     computed once per workgroup plus an immediate offset, the weights come through one buffer descriptor with the chunk in the
//     scalar offset -- no address arithmetic between the MFMAs (odd stage counts per tile: the one-stage form, WinoLoop1).
//   * epilogue: the output transform is register-local over nu; over xi the two halves exchange one 2 x 32-register
//     partial through LDS; then bias, residual, stores (8-byte, two pixels of a row) and the fused GroupNorm statistics.
//   * up-sampled input (UP): by default the zero-position variant WinoUp (conv_wino.hpp) -- 9 of the 16 positions, the raw tile
//     staged and transformed at source resolution; bit-identical to the sixteen-position form, which MCEDM_WINO_UPZ=0 keeps.
//   * images below 32 x 32 (the 16 x 16 level): the SPLIT variant WinoSplitCfg (conv_wino.hpp) -- one 32-channel block per workgroup, the sixteen
//     positions split over the eight waves, the same input path and the same expression tree in the epilogue: the bits of WinoCfg<4> / <2>.
// Results differ from the direct kernel in the last bits (a different, equally long fp32 sum: measured 1.5x its error
// against fp64, 0.1 of the rtol 1e-4 / atol 1e-5 bar); they do not depend on the batch size or the grid.
#include <atomic>
#include <cstdlib>
#include <type_traits>

#include "conv_wino.hpp"
#include "pack.hpp"
#include "prof.hpp"

namespace mcedm {

// U = G g G^T for every (cout, cin) of one weight tensor (pack.hpp wino_pack_elem)
__global__ void wino_pack_kernel(const float* __restrict__ w, float* __restrict__ dst, int Cout, int Cin, int coutp, int nch,
                                 int tflip) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= coutp * nch * WKC) return;
  wino_pack_elem(w, dst, idx, Cout, Cin, coutp, tflip);
}

// The fragment-ordered copy of a 1x1 projection's weights that the SKIP variant reads (ConvArgs::sk_wfrag): per (8-channel
// group, 32-channel output block, lane) the four k-steps of the A operand as ONE 16-byte load, like a single Winograd position
// of wino_pack_elem: f32x4[((ci / 8) * (coutp / 32) + co / 32) * 64 + (co & 31) + 32 * (ci & 1)][(ci & 7) >> 1] = w[co][ci].
__global__ void conv_frag_pack_kernel(const float* __restrict__ w, float* __restrict__ dst, int Cout, int Cin, int coutp, int cinp) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= coutp * cinp) return;
  dst[idx] = frag_pack_value(w, idx, Cout, Cin, coutp);
}

// ---- the SKIP variant's epilogue (WinoSkipCfg): the residual of a decoder block's conv1 is the 1x1 projection of the block input,
//   rv[co][px] = sk_bias[co] + sum_ci W[co][ci] * cat(sk_xa, sk_xb)[ci][px],
// and a wave's share of it -- its 32 channels x (32 patches x the two pixels of the row it stores) -- has exactly the layout of two
// 32 x 32 accumulator blocks (column = patch = lane & 31, one block per pixel of the pair), in registers that are free between the
// output transform and init_acc().  So the wave computes it: K = 2 steps over the channel pairs (2 j, 2 j + 1), j ascending, from
// the matrix pipe's zero, bias added afterwards -- conv1x1_reg_kernel's order, hence the bits of the tensor that kernel would have
// stored -- while the exchange rounds of the output transform wait behind the stage barriers of this loop instead of their own.
//   B operand: stages of 16 channels x the tile's 8 x 16 pixels = one 16-byte load per thread (thread = channel tid >> 5, row
//   (tid & 31) >> 2, column quad tid & 3 = the pixel pairs of two neighbouring patches), committed to LDS one stage later in the
//   order the MFMAs read it (conv_wino.hpp): four ds_read_b128 per stage and lane, one barrier per stage, two buffers.
//   A operand: sk_wfrag, two 16-byte loads per stage and lane, one stage ahead in registers.
template <class C, bool = C::SKIP>
struct SkipFold {};
template <class C>
struct SkipFold<C, true> {
  static constexpr int SKS = C::SKS, SKBUF = C::SKBUF, SKP = C::SKPITCH;
  __amdgpu_buffer_rsrc_t rs_a, rs_b;                      // this sample's planes of sk_xa / sk_xb (the launcher checks < 4 GiB each)
  unsigned voff, HW4;                                     // the staging load's lane offset; bytes per channel plane
  int Ca, nsk;                                            // channels of sk_xa; stages
  const f32x4* wf;
  size_t wstride;
  float* wr;                                              // LDS: where this thread commits its piece, where this lane's B fragments start
  const float* rd;
  f32x4 sld, sa[2];                                       // staged input (one stage ahead of the commit), this stage's A fragments

  __device__ __forceinline__ f32x4 req(int s) const {
    const int ci0 = SKS * s;                              // a stage lies in one source: sk_Ca % 16 == 0
    if (ci0 < Ca) return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs_a, voff, (unsigned)ci0 * HW4, 0));
    return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs_b, voff, (unsigned)(ci0 - Ca) * HW4, 0));
  }
  __device__ __forceinline__ void commit(int buf) const {
    float* d = wr + buf * SKBUF;
    *reinterpret_cast<f32x2*>(d) = f32x2{sld[0], sld[1]};
    *reinterpret_cast<f32x2*>(d + SKP) = f32x2{sld[2], sld[3]};
  }
  __device__ __forceinline__ void wreq(int s, f32x4 (&a)[2]) const {
    a[0] = wf[(size_t)(2 * s) * wstride];
    a[1] = wf[(size_t)(2 * s + 1) * wstride];
  }
  __device__ __forceinline__ void begin(const ConvArgs& p, float* skbuf, int n, int mblk, int mblocks, int y0, int x0, int tid, int lane, int hf) {
    // an opaque copy of the thread index: everything below is derived from it HERE, once per tile -- hoisted out of the stream of
    // stages these loop invariants would sit in registers through the K loop, which has none to spare (256)
    asm volatile("" : "+v"(tid));
    lane = tid & 63;
    const unsigned HW = (unsigned)p.H * (unsigned)p.W;
    HW4 = 4u * HW;
    Ca = p.sk_Ca;
    nsk = (p.sk_Ca + p.sk_Cb) / SKS;
    rs_a = make_rsrc(p.sk_xa + (size_t)n * p.sk_Ca * HW, 4u * (unsigned)p.sk_Ca * HW);
    rs_b = make_rsrc(p.sk_xb ? p.sk_xb + (size_t)n * p.sk_Cb * HW : nullptr, p.sk_xb ? 4u * (unsigned)p.sk_Cb * HW : 0u);
    const int c16 = tid >> 5, row = (tid & 31) >> 2, q = tid & 3;
    voff = 4u * ((unsigned)c16 * HW + (unsigned)(y0 + row) * (unsigned)p.W + (unsigned)(x0 + 4 * q));
    wr = skbuf + ((row & 1) * 32 + (row >> 1) * WTX + 2 * q) * SKP + (c16 & 1) * 16 + 2 * (c16 >> 1);
    rd = skbuf + (hf * 32 + (lane & 31)) * SKP + (lane >> 5) * 16;
    wf = reinterpret_cast<const f32x4*>(p.sk_wfrag) + (size_t)mblk * 64 + lane;
    wstride = (size_t)mblocks * 64;
    sld = req(0);
    wreq(0, sa);
  }
  // keep / send: the output transform's two pixel columns (conv_wino_kernel); v0 / v1 = keep + the partner's send + rv on return
  __device__ __forceinline__ void run(float* xch, const float* skb, int wave, int pw, int lane, const f32x16 (&keep)[2], const f32x16 (&send)[2],
                                      float (&v0)[16], float (&v1)[16]) {
#pragma unroll
    for (int r = 0; r < 16; ++r) xch[(wave * 16 + r) * 64 + lane] = send[0][r];
    commit(0);
    sld = req(1);                                         // nsk >= 2 (conv_wino_applicable)
    f32x16 rv[2];
    {
      const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      float z = 0.f;
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        asm volatile("" : "+v"(z));
        rv[e] = __builtin_amdgcn_mfma_f32_32x32x2f32(z, z, zero16, 0, 0, 0);
      }
    }
    __syncthreads();                                      // stage 0 and round 0 of the exchange are in LDS
#pragma unroll
    for (int r = 0; r < 16; ++r) v0[r] = keep[0][r] + xch[(pw * 16 + r) * 64 + lane];
    f32x4 bq[4];
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) bq[jj] = *reinterpret_cast<const f32x4*>(rd + 4 * jj);
    for (int s = 0; s < nsk; ++s) {
      f32x4 bqn[4], san[2];
      wreq(s + 1 < nsk ? s + 1 : s, san);
      // stage s + 1 goes to the buffer that stage s - 1 was read from (before the last barrier), stage s + 2 is requested; past the
      // end both repeat the last stage (a buffer nobody reads, a load nobody uses): no branch
      commit((s + 1) & 1);
      sld = req(s + 2 < nsk ? s + 2 : nsk - 1);
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int e = 0; e < 2; ++e) rv[e] = __builtin_amdgcn_mfma_f32_32x32x2f32(sa[j >> 2][j & 3], bq[j >> 1][2 * (j & 1) + e], rv[e], 0, 0, 0);
      // the stage barrier sits in the MIDDLE of the stage's MFMAs: the next stage's fragments are read right behind it and
      // arrive under the second half (behind a barrier at the end of the stage both waves of a SIMD wait for LDS together;
      // measured 45.8 k -> 45.1 k cycles per tile for the phase)
      __syncthreads();
      const float* b = rd + ((s + 1) & 1) * SKBUF;
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) bqn[jj] = *reinterpret_cast<const f32x4*>(b + 4 * jj);
      // the exchange rounds ride on these barriers: every wave read round 0 before its first MFMA, so round 1 may be written
      // behind the first stage barrier and read behind the second
      if (s == 0) {
#pragma unroll
        for (int r = 0; r < 16; ++r) xch[(wave * 16 + r) * 64 + lane] = send[1][r];
      }
      if (s == 1) {
#pragma unroll
        for (int r = 0; r < 16; ++r) v1[r] = keep[1][r] + xch[(pw * 16 + r) * 64 + lane];
      }
#pragma unroll
      for (int j = 4; j < 8; ++j)
#pragma unroll
        for (int e = 0; e < 2; ++e) rv[e] = __builtin_amdgcn_mfma_f32_32x32x2f32(sa[j >> 2][j & 3], bq[j >> 1][2 * (j & 1) + e], rv[e], 0, 0, 0);
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) bq[jj] = bqn[jj];
      sa[0] = san[0];
      sa[1] = san[1];
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float bs = skb[(r & 3) + 8 * (r >> 2)];
      v0[r] = v0[r] + (rv[0][r] + bs);
      v1[r] = v1[r] + (rv[1][r] + bs);
    }
  }
};

// LDS accesses of the K loop by byte address: a per-lane base that sits in a register through the loop plus an offset that is a
// compile-time constant wherever the buffer parity is one (the two-stage trip): hipcc then puts it into the instruction's 16-bit
// offset field instead of adding it to the lane index in front of every group of accesses.
template <class T>
__device__ __forceinline__ T lds_get(unsigned base, int off) {
  return *reinterpret_cast<const __attribute__((address_space(3))) T*>(base + (unsigned)off);
}
template <class T>
__device__ __forceinline__ void lds_put(unsigned base, int off, T v) {
  *reinterpret_cast<__attribute__((address_space(3))) T*>(base + (unsigned)off) = v;
}
// The input transform's packed fp32 operations, written as instructions.  Behind an MFMA hipcc rewrites a v_pk_add / v_pk_fma_f32 into two
// scalar instructions after register allocation (it takes the matrix instruction's shadow for free issue slots); on gfx950 vector and
// fp32 matrix instructions do not overlap, so the rewrite doubles what the operation costs -- fifteen of the stage's sixteen were split.
// Same operations on the same values: a + (-b) for a - b, and c1 + c2 | c1 - c2 for the fma with (1, -1), whose product is exact.
__device__ __forceinline__ f32x2 pk_sub(f32x2 a, f32x2 b) {
  f32x2 d;
  asm("v_pk_add_f32 %0, %1, %2 neg_lo:[0,1] neg_hi:[0,1]" : "=v"(d) : "v"(a), "v"(b));
  return d;
}
__device__ __forceinline__ f32x2 pk_fma(f32x2 a, f32x2 b, f32x2 c) {
  f32x2 d;
  asm("v_pk_fma_f32 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "v"(c));
  return d;
}
// (a.y + b.x, a.y - b.x)
__device__ __forceinline__ f32x2 pk_hi_pm_lo(f32x2 a, f32x2 b) {
  f32x2 d;
  asm("v_pk_add_f32 %0, %1, %2 op_sel:[1,0] op_sel_hi:[1,0] neg_hi:[0,1]" : "=v"(d) : "v"(a), "v"(b));
  return d;
}
// half_sum32 (conv_tile.hpp: the sum over the 32 lanes of a half-wave, in every lane) with its last step in registers: behind the four
// DPP steps every lane of a 16-lane row holds its row's sum, and v_permlane16_swap_b32 exchanges the odd rows of one copy with the even
// rows of another -- row pair (0, 1) | (2, 3): a = (s0, s0, s2, s2), b = (s1, s1, s3, s3) -- so a + b adds the same two partial sums as
// v + __shfl_xor(v, 16) did (s0 + s1 in row 0, s1 + s0 in row 1: the same bits) without the ds_bpermute_b32 round trip through the
// LDS pipe and its wait.  Written as an instruction with BOTH operands read-write (the builtin lost its second result here,
// DESIGN.md section 3); the two wait states a vector write of either operand needs in front of it are inside the string.
__device__ __forceinline__ float half_sum32_swap(float v) {
#define MCEDM_DPP(x, ctrl) __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), ctrl, 0xf, 0xf, true))
  v += MCEDM_DPP(v, 0xB1);       // quad_perm [1, 0, 3, 2]
  v += MCEDM_DPP(v, 0x4E);       // quad_perm [2, 3, 0, 1]
  v += MCEDM_DPP(v, 0x141);      // row_half_mirror
  v += MCEDM_DPP(v, 0x140);      // row_mirror
#undef MCEDM_DPP
  float a = v, b = v;
  asm("s_nop 1\n\tv_permlane16_swap_b32 %0, %1" : "+v"(a), "+v"(b));
  return a + b;
}
// the largest immediate offset of an LDS access family (bytes; the last byte of the access) must fit the instruction's field
#define WINO_LDS_IMM_OK(floats, bytes) static_assert(4 * (floats) + (bytes) <= 65536, "LDS offset beyond the 16-bit immediate field")

// UP: the conv input is the nearest-neighbour 2x up-sampling of the (activated) source (adm_blocks.py:69-73)
// ACT = false: the launch has no activation (p.act == 0: the data-gradient convs of training, whose input is a raw gradient): the
// plain variant's branch-free "evaluate SiLU and select" is compiled out -- ~20 of the ~58 vector instructions per chunk and lane,
// every one of them matrix time (round 5; the forward convs of inference all carry the activation)
// Tag: empty, or WinoUp<SRC> (conv_wino.hpp): the zero-position variant of the up-sampling kernel; WinoLoop1 in front: one stage per trip
template <class C, bool UP, bool ACT = true, class... Tag>
__global__ __launch_bounds__(C::NT, C::MB == 4 ? 1 : 2) void conv_wino_kernel(const ConvArgs p, int tiles_x, int tiles_img, int nch, int mblocks,
                                                                          int per, int mode) {
  constexpr int WSC = C::SC, VBUF = C::VBUF, RBUF = C::RBUF, MB = C::MB;
  constexpr bool SKIP = C::SKIP;                                  // WinoSkipCfg: the epilogue computes the residual (the skip projection)
  constexpr bool UPZ = WinoUpTraits<Tag...>::UPZ;                 // WinoUp: nothing is done for the positions whose V is exactly +0
  constexpr bool UPS = WinoUpTraits<Tag...>::UPS;                 // ... and the raw tile is staged and transformed at source resolution
  constexpr bool PAIR = !WinoUpTraits<Tag...>::LOOP1;             // two stages per trip, immediate LDS offsets, buffer descriptors (WinoLoop1: not)
  static_assert(!UPS || UPZ, "source-resolution staging is part of the zero-position variant");
  static_assert(!UPZ || (UP && !SKIP), "the zero positions belong to the up-sampled input");
  constexpr bool SPLIT = C::SPLIT;                                // WinoSplitCfg: one 32-channel block per workgroup, the positions split over the waves
  static_assert(!SPLIT || (!UP && !SKIP && !UPZ && !WinoUpTraits<Tag...>::BROWS && MB == 4 && WSC == 2), "the split variant: plain input, WinoCfg<4>'s input path");
  extern __shared__ float lds[];
  const int Cin = p.Ca + p.Cb;
  Coef* const cfl = reinterpret_cast<Coef*>(lds + C::LDS_ROWS_OFF);
  float* const xch = lds + C::LDS_ROWS_OFF + 4 * Cin;            // epilogue exchange (one 16-register round), then the records
  float* const red = xch + C::XCH_FLOATS;
  float* const bias_l = red + 2 * (C::MT / 2) * 3;                // this workgroup's MT bias values
  float* const skb_l = bias_l + C::MT;                            // SKIP: the projection's MT bias values, then its two stage buffers
  float* const skbuf = skb_l + C::MT;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int mb = wave % MB, hf = wave / MB;
  // the K loop's LDS accesses: byte addresses (lds_get / lds_put); RB0: where rbuf starts
  const unsigned lds0 = (unsigned)reinterpret_cast<size_t>((__attribute__((address_space(3))) float*)lds);
  constexpr int RB0 = 4 * 2 * VBUF;
  if (p.dbg && tid == 0) { p.dbg[blockIdx.x * 16 + 0] = __builtin_amdgcn_s_memrealtime(); p.dbg[blockIdx.x * 16 + 4] = per; }
  // A workgroup takes `per` consecutive pixel tiles of ONE sample (the launcher picks a divisor of the tiles per image) and
  // runs their stages as one stream: the pipeline below never drains between tiles, only the accumulators are written out.
  // mode bit 256 (round 5, MCEDM_WINO_MAP): the tiles_img / per workgroups of a sample share an XCD (ids 8 apart: one L2) and walk the
  // image INTERLEAVED -- workgroup j takes tiles j, j + wps, ... -- so that at any time they work on neighbouring tiles and fetch each
  // other's halo columns out of that L2 (with consecutive tiles per workgroup a tile's 24 x 10 fetch per 16 x 8 pixels had left the
  // 4 MB L2 long before the neighbouring tile asked for its overlap: 1.9x the input from HBM).  Same tiles, same sums: same bits.
  int gt0 = blockIdx.x * per, tstep = 1;
  int n = gt0 / tiles_img, tile0 = gt0 % tiles_img;
  if (!SPLIT && (mode & 256)) {
    const int nwg = gridDim.x, wps = tiles_img / per;
    const int lid = (nwg % 8 == 0) ? (int)(blockIdx.x % 8) * (nwg / 8) + (int)(blockIdx.x / 8) : (int)blockIdx.x;
    n = lid / wps; tile0 = lid % wps; tstep = wps;
  }
  // SPLIT: a 1-D grid of B x tiles x Cout / 32 workgroups, one tile each; the Cout / 32 workgroups of a tile are consecutive in `lid`,
  // i.e. 8 apart in workgroup id: one XCD, so that they find the raw tile and the producers' statistics in one L2
  int split_mb = 0;
  if constexpr (SPLIT) {
    const int nwg = gridDim.x, nmb = p.Cout / C::MT;
    const int lid = (nwg % 8 == 0) ? (int)(blockIdx.x % 8) * (nwg / 8) + (int)(blockIdx.x / 8) : (int)blockIdx.x;
    split_mb = lid % nmb;
    n = (lid / nmb) / tiles_img; tile0 = (lid / nmb) % tiles_img;
  }
  const int m0 = SPLIT ? split_mb * C::MT : blockIdx.y * C::MT;
  const size_t HW = (size_t)p.H * p.W, HWs = (size_t)p.Hs * p.Ws;
  const int nst = (nch + WSC - 1) / WSC;                           // stages per tile
  const int G = per * nst;                                        // stages of this workgroup

  // ---- raw staging: wave w stages channels w CPW .. of every chunk: a channel's 10 x 18 patch (tile + halo).
  //   plain input: ONE 16-byte load per lane and channel -- lane = (patch row r = lane / 6, aligned quad lane % 6 of the 24
  //   columns x0 - 4 .. x0 + 19): vector-memory instructions are the expensive thing in this loop (~60 cycles of issue
  //   each), and the 6 columns fetched beyond the patch cost two extra SiLU evaluations per lane instead;
  //   up-sampled input: elements lane, lane + 64, lane + 128 of the 180, one dword load each (source pixel (y/2, x/2)).
  // Geometry (byte offsets, zero-padding masks) of the tile that is being LOADED; the masks of the tile whose registers are
  // waiting to be COMMITTED are kept beside them (the two differ for one trip at a tile boundary).
  //   UPS: element `lane` of the 6 x 10 source patch, one dword load.
  constexpr int NR = UPS ? 1 : UP ? RSUB : 4, NG = UPS ? 1 : UP ? RSUB : 1;   // raw registers / geometry entries per lane and channel
  unsigned roff[NG], rkeepL[NG], rkeepC[NG];
  // where this lane commits in the raw tile's LDS plane of the wave's first channel (byte addresses, opaque to the compiler: they stay
  // in these registers through the loop).  Plain input: the quad's four elements; up-sampled input: element `lane`
  constexpr int NCM = UP ? 1 : 4;
  unsigned cm_a[NCM];
  if (!UP) {
    const int r = lane / 6, qd = lane % 6;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int col = 4 * qd + e - 3;                              // column inside the 18-wide patch; -3 .. -1 and 18 .. 20 are not part of it
      const int lofs = (lane < 60 && col >= 0 && col < RPITCH) ? r * RPITCH + col : RROWS * RPITCH + lane % (RPLANE - RROWS * RPITCH);
      cm_a[e] = lds0 + RB0 + 4 * (wave * C::CPW * RPLANE + lofs);
    }
  } else {
    cm_a[0] = lds0 + RB0 + 4 * (wave * C::CPW * (UPS ? UPLANE : RPLANE) + lane);
  }
#pragma unroll
  for (int e = 0; e < NCM; ++e) asm volatile("" : "+v"(cm_a[e]));
  WINO_LDS_IMM_OK(RBUF + ((WSC - 1) * WKC + C::CPW - 1) * RPLANE + (UP && !UPS ? 64 * (RSUB - 1) : 0), 4);      // the commit's stores
  auto set_geom = [&](int tile) {
    const int y0 = (tile / tiles_x) * WPH, x0 = (tile % tiles_x) * WPW;
    if (UPS) {     // zero padding = source row / column -1 or Hs / Ws (H = 2 Hs, W = 2 Ws, y0 and x0 even)
      const int r = lane / UCOLS, c = lane - r * UCOLS;
      const int y = (y0 >> 1) - 1 + r, x = (x0 >> 1) - 1 + c;
      const bool inb = lane < UROWS * UCOLS && (unsigned)y < (unsigned)p.Hs && (unsigned)x < (unsigned)p.Ws;
      rkeepL[0] = inb ? 0xffffffffu : 0u;
      roff[0] = !inb ? 0u : 4u * (unsigned)(y * p.Ws + x);
    } else if (UP) {
#pragma unroll
      for (int i = 0; i < NG; ++i) {
        const int e = lane + 64 * i;
        const int r = e / RPITCH, c = e - r * RPITCH;
        const int y = y0 - 1 + r, x = x0 - 1 + c;
        const bool inb = e < RROWS * RPITCH && (unsigned)y < (unsigned)p.H && (unsigned)x < (unsigned)p.W;
        rkeepL[i] = inb ? 0xffffffffu : 0u;
        roff[i] = !inb ? 0u : 4u * (unsigned)((y >> 1) * p.Ws + (x >> 1));
      }
    } else {       // W % 16 == 0 and x0 % 16 == 0: a quad lies wholly inside or wholly outside the image, and is 16-byte aligned
      const int y = y0 - 1 + lane / 6, x = x0 - 4 + 4 * (lane % 6);
      const bool inb = lane < 60 && (unsigned)y < (unsigned)p.H && x >= 0 && x < p.W;
      rkeepL[0] = inb ? 0xffffffffu : 0u;
      roff[0] = inb ? 4u * (unsigned)(y * p.W + x) : 0u;
    }
  };
  float raw[WSC][C::CPW][NR];
  int ld_st = 0, ld_tile = tile0, cm_st = 0;                       // stage (within its tile) of the next load / commit
  set_geom(tile0);
  auto raw_load1 = [&](int sc) {
#pragma unroll
    for (int cw = 0; cw < C::CPW; ++cw) {
      const int ci = (ld_st * WSC + sc) * WKC + wave * C::CPW + cw;
      const bool in_a = ci < p.Ca;
      const float* src = in_a ? p.xa : p.xb;
      const int cc = in_a ? ci : ci - p.Ca, CC = in_a ? p.Ca : p.Cb;
      const bool ok = ci < Cin && src != nullptr;
      const float* plane = ok ? src + ((size_t)n * CC + cc) * HWs : (p.xa ? p.xa : p.xb);
      if (UP) {
#pragma unroll
        for (int i = 0; i < NG; ++i) raw[sc][cw][i] = *reinterpret_cast<const float*>(reinterpret_cast<const char*>(plane) + roff[i]);
      } else {
        const f32x4 q = *reinterpret_cast<const f32x4*>(reinterpret_cast<const char*>(plane) + roff[0]);
#pragma unroll
        for (int e = 0; e < 4; ++e) raw[sc][cw][e] = q[e];
      }
    }
  };
  auto raw_load_next = [&]() { if (++ld_st == nst) { ld_st = 0; ld_tile += tstep; set_geom(ld_tile < tiles_img ? ld_tile : tiles_img - 1); } };
  auto raw_load_done = [&]() {                                     // all chunks of the stage requested: on to the next stage
#pragma unroll
    for (int i = 0; i < NG; ++i) rkeepC[i] = rkeepL[i];            // these registers are committed one trip from now
  };
  auto raw_load = [&]() {                                          // the next stage of the stream
#pragma unroll
    for (int sc = 0; sc < WSC; ++sc) raw_load1(sc);
    raw_load_done();
    raw_load_next();
  };
  // The transform of a lane's four elements is written on PAIRS (v_pk_add / v_pk_fma / v_pk_mul_f32: two elements per vector
  // instruction) and the zero padding is folded into the lane's copy of the row -- (v - mean) * 0 + 0 --: vector instructions
  // do not overlap with the fp32 MFMAs of either wave of the SIMD, so every one removed from this loop is
  // matrix time.  Same operations in the same order as apply_coef(): bit-identical values.
  auto raw_commit1 = [&](int sc, int rbo) {                         // rbo: byte offset of the raw buffer (parity * RBUF)
#pragma unroll
    for (int cw = 0; cw < C::CPW; ++cw) {
      const int kl = wave * C::CPW + cw, ci = (cm_st * WSC + sc) * WKC + kl;
      const bool ok = ci < Cin && (ci < p.Ca ? p.xa : p.xb) != nullptr;
      const Coef cf = cfl[ci < Cin ? ci : Cin - 1];
      const unsigned ck = ok ? 0xffffffffu : 0u;
      if (UPS) {
        float v = apply_coef(raw[sc][cw][0], cf, p.act);
        v = __builtin_bit_cast(float, __builtin_bit_cast(unsigned, v) & (rkeepC[0] & ck));
        lds_put(cm_a[0], rbo + 4 * (sc * WKC + cw) * UPLANE, v);     // lanes 60 .. 63: zeros into the plane's pad
      } else if (UP) {
#pragma unroll
        for (int i = 0; i < NR; ++i) {
          float v = apply_coef(raw[sc][cw][i], cf, p.act);
          v = __builtin_bit_cast(float, __builtin_bit_cast(unsigned, v) & (rkeepC[i] & ck));
          if (i + 1 < RSUB || lane + 64 * i < RROWS * RPITCH) lds_put(cm_a[0], rbo + 4 * ((sc * WKC + cw) * RPLANE + 64 * i), v);
        }
      } else {
        // zero padding = (v - mean) * 0 + 0 on the lane's copy of the row.  PRECONDITION: finite activations -- an out-of-image
        // lane loads element 0 of the plane, and an Inf / NaN there (or a (v - mean) that overflows) would make the padding NaN
        // instead of 0; the up-sampling variant above masks the finished value bit-wise.  (A network whose activations are
        // not finite has no meaningful output either way; two v_and per pair here would cost ~3 % of the slice's vector work.)
        // PRECONDITION of the zero-position variant (WinoUp, conv_wino.hpp): finite transformed WEIGHTS -- a product with an
        // exactly zero V is dropped there, where the sixteen-position kernel would have turned 0 * Inf into NaN.
        const unsigned mk = rkeepC[0] & ck;
        const float scm = __builtin_bit_cast(float, __builtin_bit_cast(unsigned, cf.scale) & mk);
        const float ofm = __builtin_bit_cast(float, __builtin_bit_cast(unsigned, cf.offset) & mk);
        f32x2 t[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const f32x2 v = {raw[sc][cw][2 * h], raw[sc][cw][2 * h + 1]};
          t[h] = (v - cf.mean) * scm + ofm;
        }
        // no branch (a slot must stay ONE basic block, see the K loop): the activation is a template parameter
#pragma unroll
        for (int h = 0; h < 2; ++h) { if constexpr (ACT) t[h] = silu_f2(t[h]); }       // ACT == (p.act != 0): the launcher's choice
#pragma unroll
        for (int i = 0; i < 4; ++i) lds_put(cm_a[UP ? 0 : i], rbo + 4 * (sc * WKC + cw) * RPLANE, (float)t[i >> 1][i & 1]);
      }
    }
  };
  auto commit_done = [&]() { if (++cm_st == nst) cm_st = 0; };
  // ---- input transform: thread = (channel k, patch (ty, tx), row half hf): V[xi][nu] for xi in {2 hf, 2 hf + 1}.
  // In two halves (LDS reads / arithmetic + LDS writes) per chunk of the stage, so that the K loop can spread them out.
  // patch rows ty = mb + MB ti, ti < TI
  // B^T = [[1,0,-1,0],[0,1,1,0],[0,-1,1,0],[0,1,0,-1]] down the rows r0 .. r3 of the 4 x 4 patch.  Both halves evaluate ONE
  // formula, t0 = Y - X, t1 = X + s Z (no per-half selects): hf = 0: (Y, Z, X, s) = (r0, r1, r2, +1) gives (r0 - r2, r1 + r2),
  // hf = 1: (r2, r3, r1, -1) gives (r2 - r1, r1 - r3); the halves differ in two LDS row offsets and a sign.  Along the columns
  // (o0, o3) = (c0, c1) - (c2, c3) and (o1, -o2) = (c1, c1) + (c2, -c2): two packed additions per row; nu = 2 is stored negated
  // and the packed weights carry the same sign (wino_pack_kernel).  8 packed vector instructions per chunk and thread.
  const int tk = lane & 7, ttx = lane >> 3, tty = mb;
  // rows Y / Z and row X of this thread's patch in the raw tile, its first V element: byte addresses like cm_a
  unsigned tr_yz = lds0 + RB0 + 4 * (UPS ? tk * UPLANE + (tty + hf) * UCOLS + ttx : tk * RPLANE + (2 * tty + 2 * hf) * RPITCH + 2 * ttx);
  unsigned tr_x = lds0 + RB0 + 4 * (UPS ? tk * UPLANE + (tty + 1) * UCOLS + ttx : tk * RPLANE + (2 * tty + 2 - hf) * RPITCH + 2 * ttx);
  const float tsgn = hf ? -1.f : 1.f;
  const f32x2 tsgn2 = {tsgn, tsgn};
  unsigned tr_dst = lds0 + 4 * ((8 * hf) * VPOS + (tk & 1) * VH1 + (tty * WTX + ttx) * 4 + (tk >> 1));
  asm volatile("" : "+v"(tr_yz), "+v"(tr_x), "+v"(tr_dst));
  WINO_LDS_IMM_OK(RBUF + (WSC - 1) * WKC * (UPS ? UPLANE : RPLANE) + (C::TI - 1) * MB * (UPS ? UCOLS : 2 * RPITCH) + (UPS ? UCOLS + 2 : RPITCH + 2), UPS ? 4 : 8);   // its reads
  WINO_LDS_IMM_OK(VBUF + (WSC - 1) * 16 * VPOS + (C::TI - 1) * MB * WTX * 4 + 7 * VPOS, 4);                                                  // its stores
  f32x2 td[WSC][C::TI][3][2];                         // rows Y, Z, X; column pairs (c0, c1), (c2, c3)
  // UPS: the same rows out of the source patch -- patch row r = source row (r + 1) >> 1: Y = ty + hf, Z = ty + 1 + hf, X = ty + 1 -- and
  // the three source columns tx, tx + 1, tx + 2 = (c0, c1 = c2, c3)
  float tu[WSC][C::TI][3][3];
  auto transform_read1 = [&](int sc, int rbo) {                     // rbo, vbo: byte offsets of the raw / V buffer (parity * RBUF, * VBUF)
    if constexpr (UPS) {
#pragma unroll
      for (int ti = 0; ti < C::TI; ++ti) {
        const int b = rbo + 4 * (sc * WKC * UPLANE + MB * ti * UCOLS);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          tu[sc][ti][0][c] = lds_get<float>(tr_yz, b + 4 * c);
          tu[sc][ti][1][c] = lds_get<float>(tr_yz, b + 4 * (UCOLS + c));
          tu[sc][ti][2][c] = lds_get<float>(tr_x, b + 4 * c);
        }
      }
      return;
    }
#pragma unroll
    for (int ti = 0; ti < C::TI; ++ti)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int b = rbo + 4 * (sc * WKC * RPLANE + 2 * MB * ti * RPITCH + 2 * j);
        td[sc][ti][0][j] = lds_get<f32x2>(tr_yz, b);
        td[sc][ti][1][j] = lds_get<f32x2>(tr_yz, b + 4 * RPITCH);
        td[sc][ti][2][j] = lds_get<f32x2>(tr_x, b);
      }
  };
  auto transform_finish1 = [&](int sc, int vbo) {
    if constexpr (UPS) {
#pragma unroll
      for (int ti = 0; ti < C::TI; ++ti) {
        float t[2][3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          t[0][c] = tu[sc][ti][0][c] - tu[sc][ti][2][c];
          t[1][c] = tu[sc][ti][2][c] + tsgn * tu[sc][ti][1][c];
        }
#pragma unroll
        for (int x = 0; x < 2; ++x) {
          if (x == 0 && hf != 0) continue;                 // xi = 2 of the hf = 1 waves is exactly +0 and nobody reads it
          const int o = vbo + 4 * (sc * 16 * VPOS + MB * ti * WTX * 4 + 4 * x * VPOS);
          lds_put(tr_dst, o + 4 * 0 * VPOS, t[x][0] - t[x][1]);            // c0 - c2
          lds_put(tr_dst, o + 4 * 1 * VPOS, t[x][1] + 1.f * t[x][1]);      // c1 + c2
          lds_put(tr_dst, o + 4 * 3 * VPOS, t[x][1] - t[x][2]);            // c1 - c3
        }
      }
      return;
    }
#pragma unroll
    for (int ti = 0; ti < C::TI; ++ti) {
      f32x2 t[2][2];
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        t[0][j] = pk_sub(td[sc][ti][0][j], td[sc][ti][2][j]);
        t[1][j] = pk_fma(tsgn2, td[sc][ti][1][j], td[sc][ti][2][j]);
      }
#pragma unroll
      for (int x = 0; x < 2; ++x) {
        const f32x2 o03 = pk_sub(t[x][0], t[x][1]);
        const f32x2 o12 = pk_hi_pm_lo(t[x][0], t[x][1]);       // (c1 + c2, c1 - c2)
        const int o = vbo + 4 * (sc * 16 * VPOS + MB * ti * WTX * 4 + 4 * x * VPOS);
        lds_put(tr_dst, o + 4 * 0 * VPOS, (float)o03.x);
        lds_put(tr_dst, o + 4 * 1 * VPOS, (float)o12.x);
        if constexpr (!UPZ) lds_put(tr_dst, o + 4 * 2 * VPOS, (float)o12.y);   // UPZ: nu = 2 is exactly +0 and nobody reads it
        lds_put(tr_dst, o + 4 * 3 * VPOS, (float)o03.y);
      }
    }
  };
  auto transform_read = [&](int rbo) { for (int sc = 0; sc < WSC; ++sc) transform_read1(sc, rbo); };
  auto transform_finish = [&](int vbo) { for (int sc = 0; sc < WSC; ++sc) transform_finish1(sc, vbo); };

  // ---- prologue (once per workgroup): transform rows of the sample, stages 0 .. 2 of the stream
  stage_coef_rows<C::NT>(p, n, cfl, tid);
  if (tid < C::MT) bias_l[tid] = p.bias ? p.bias[(WinoUpTraits<Tag...>::BROWS ? n * p.bias_batch : 0) + m0 + tid] : 0.f;
  if constexpr (SKIP) { if (tid < C::MT) skb_l[tid] = p.sk_bias ? p.sk_bias[m0 + tid] : 0.f; }
  raw_load();
  __syncthreads();
  for (int sc = 0; sc < WSC; ++sc) raw_commit1(sc, 0);
  commit_done();
  if (G > 1) { raw_load(); for (int sc = 0; sc < WSC; ++sc) raw_commit1(sc, 4 * RBUF); commit_done(); }
  if (G > 2) raw_load();                                             // stays in registers until trip 0 commits it
  // this wave's transformed weights: 8 positions x one 16-byte load per chunk
  const size_t ustride = (size_t)mblocks * 16 * 64;                  // f32x4 per chunk
  // UPZ: block q of the hf = 1 waves is position 12 + q (xi = 3 first; its blocks 4 .. 7, xi = 2, are never touched)
  constexpr int PHF = UPZ ? 12 : 8;                                  // first position of the hf = 1 waves' block 0
  // SPLIT: the wave's two positions 2 wave, 2 wave + 1 of the workgroup's block
  const size_t upos = (SPLIT ? ((size_t)(m0 / 32) * 16 + 2 * wave) : ((size_t)(m0 / 32 + mb) * 16 + PHF * hf)) * 64 + lane;   // f32x4 index inside a chunk
  const f32x4* up = reinterpret_cast<const f32x4*>(p.wino) + upos;
  // PAIR: ONE descriptor over the table (the launcher checks < 4 GiB), the lane's offset fixed for the kernel, the chunk in the scalar
  // offset operand: no 64-bit pointer arithmetic per chunk.  The instruction's offset field is 12 bits, blocks 4 .. 7 lie 4096 ..
  // 7168 bytes behind block 0: uw[1] = uw[0] + 4096 (the register the pointer's high half had) serves them.
  const unsigned ustride_b = 16u * (unsigned)ustride;                // bytes per chunk
  const __amdgpu_buffer_rsrc_t rs_w = make_rsrc(PAIR ? p.wino : nullptr, PAIR ? (unsigned)nch * ustride_b : 0u);
  unsigned uw[2] = {16u * (unsigned)upos, 16u * (unsigned)upos + 4096u};
  if constexpr (PAIR) asm volatile("" : "+v"(uw[0]), "+v"(uw[1]));
  auto wfrag = [&](int chunk, int q) -> f32x4 {                      // block q of this wave's positions, of chunk `chunk` (wave-uniform)
    if constexpr (PAIR) {
      // the lane offset is "redefined" in front of every load (no instruction): lane offset + block stays ONE use of a fresh value, which the
      // load takes as register + immediate -- left loop-invariant, hipcc keeps a register per block through the loop (six more, and spills)
      asm("" : "+v"(uw[q >> 2]));
      return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs_w, uw[q >> 2] + (unsigned)(q & 3) * 1024u, (unsigned)chunk * ustride_b, 0));
    } else {
      return up[(size_t)chunk * ustride + q * 64];
    }
  };
  f32x4 ua[8];                                                       // reloaded position by position right after its last use
  // SPLIT: [chunk of the stage][position]: the current stage's fragments; the next stage's are requested a whole stage ahead
  // (registers are plentiful here) and past the last chunk of the tile comes chunk 0 again, as in the other variants
  f32x4 wa[WSC][2];
  if constexpr (SPLIT) {
#pragma unroll
    for (int sc = 0; sc < WSC; ++sc)
#pragma unroll
      for (int q = 0; q < 2; ++q) wa[sc][q] = wfrag(sc < nch ? sc : 0, q);
  } else if constexpr (UPZ) {
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    ua[0] = wfrag(0, 0); ua[1] = wfrag(0, 1); ua[3] = wfrag(0, 3);
    ua[4] = zero4; ua[5] = zero4; ua[7] = zero4;
    if (hf == 0) { ua[4] = wfrag(0, 4); ua[5] = wfrag(0, 5); ua[7] = wfrag(0, 7); }
  } else {
#pragma unroll
    for (int q = 0; q < 8; ++q) ua[q] = wfrag(0, q);
  }
  __syncthreads();
  transform_read(0);
  transform_finish(0);
  // Accumulators start at zero, except Winograd position (xi, nu) = (1, 1) -- block 5 of the hf = 0 waves --, which starts at
  // the bias: A^T has ones in column 1 of both rows, so a constant there comes out as that constant in all four pixels.
  // Zeroing is done by the matrix pipe itself -- D = 0 * 0 + 0 with the inline constant as C: eight instructions (512 cycles)
  // instead of 128 v_mov: the in-kernel stamps put the v_mov version at 3500 cycles per tile with both waves of a SIMD in it
  // (a wave issues a vector instruction every ~7 cycles at best here).
  f32x16 acc[8];
  auto init_acc = [&]() {
    const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float z = 0.f;
#pragma unroll
    for (int q = 0; q < (SPLIT ? 2 : 8); ++q) {
      asm volatile("" : "+v"(z));                          // an opaque zero per block: eight matrix instructions, not one + 112 copies
      acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(z, z, zero16, 0, 0, 0);
    }
    if constexpr (SPLIT) {                                 // position (1, 1) = 5 is block 1 of wave 2
      if (wave == 2) {
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[1][r] = bias_l[4 * (lane >> 5) + (r & 3) + 8 * (r >> 2)];
      }
    } else if (hf == 0) {
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[5][r] = bias_l[32 * mb + 4 * (lane >> 5) + (r & 3) + 8 * (r >> 2)];
    }
  };
  __syncthreads();
  init_acc();

  // ---- the stream of stages: one trip = one stage of WSC chunks
  unsigned vrd = lds0 + 4 * ((SPLIT ? 2 * wave : PHF * hf) * VPOS + (lane >> 5) * VH1 + (lane & 31) * 4);   // this lane's B fragment of block 0: a byte address like cm_a
  asm volatile("" : "+v"(vrd));
  WINO_LDS_IMM_OK(VBUF + (WSC - 1) * 16 * VPOS + 7 * VPOS, 16);
  if (p.dbg && tid == 0) { p.dbg[blockIdx.x * 16 + 1] = __builtin_amdgcn_s_memrealtime(); p.dbg[blockIdx.x * 16 + 5] = __builtin_amdgcn_s_memtime(); }
#ifdef MCEDM_WINO_TIMELINE      // cycle sums of waves 0 and MB (lane 0): MFMA stream, barrier, epilogue -> dbg[8..12] / dbg[13..15, 7] (diagnostic builds only)
  unsigned long long ph[5] = {0, 0, 0, 0, 0}, tlast = __builtin_amdgcn_s_memtime();
#define WINO_STAMP(i) { const unsigned long long t_ = __builtin_amdgcn_s_memtime(); ph[i] += t_ - tlast; tlast = t_; }
  unsigned long long sl[8] = {0, 0, 0, 0, 0, 0, 0, 0}, slast = 0;      // mode bit 16: cycles per slot of the stage (wave 0) -> dbg[8..15]
#define WINO_SLOT(i) { const unsigned long long t_ = __builtin_amdgcn_s_memtime(); sl[(i) & 7] += t_ - slast; slast = t_; }
#define WINO_SLOT0 { slast = __builtin_amdgcn_s_memtime(); }
  unsigned long long ep[6] = {0, 0, 0, 0, 0, 0}, elast = 0;          // mode bit 32: cycles per phase of the epilogue (wave 0) -> dbg[8..13]
#define WINO_EP(i) { __builtin_amdgcn_sched_barrier(0); const unsigned long long t_ = __builtin_amdgcn_s_memtime(); if (i) ep[(i) - 1] += t_ - elast; elast = t_; __builtin_amdgcn_sched_barrier(0); }
  const bool no_u = mode & 2;                                       // drop the weight reloads (wrong results; ablation)
#else
#define WINO_STAMP(i)
#define WINO_SLOT(i)
#define WINO_SLOT0
#define WINO_EP(i)
  constexpr bool no_u = false;
#endif
  // One trip = one stage: WSC x 4 slots of [two B-fragment reads for the next slot | eight MFMAs | two weight reloads] and,
  // behind each slot's MFMAs, one slice of the side work that prepares later stages -- the transform of stage g + 1 (LDS
  // reads in slots 0 / 3, arithmetic + LDS writes in slots 2 / 5), the commit of the raw tile of stage g + 2 (slots 1 / 4; its
  // global loads were issued a trip ago) and the loads of stage g + 3 (slot 6); stages past the end of a tile are the first
  // stages of the workgroup's next tile.  Sliced like this the side work costs its issue cycles; as a phase of its own
  // (before or after the MFMAs, or ping-ponged between the two waves of a SIMD) it cost its latencies: 2400 cycles per chunk
  // and wave against 2048 of MFMAs.  Every slice touches buffers no MFMA of this trip reads: one barrier per trip.
  // UPZ: a chunk is THREE slots of four MFMAs -- the blocks 0, 1, 3 that both halves run -- and behind them, for the hf = 0 waves
  // only, the twelve MFMAs of blocks 4, 5, 7 with their B reads and reloads behind ONE wave-uniform branch: no side work in there
  // (a second copy of a slice is what makes hipcc give the accumulators a second register set), so the six
  // slices of a stage sit in its six common slots, ten instructions behind each MFMA instead of five.
  auto side_slice_upz = [&](int slot, int cur) {
    if (WSC == 2) {
      if (slot == 0) transform_read1(0, 4 * (cur ^ 1) * RBUF);
      if (slot == 1) raw_commit1(0, 4 * cur * RBUF);
      if (slot == 2) { transform_finish1(0, 4 * (cur ^ 1) * VBUF); raw_load1(0); }
      if (slot == 3) transform_read1(WSC - 1, 4 * (cur ^ 1) * RBUF);
      if (slot == 4) { raw_commit1(WSC - 1, 4 * cur * RBUF); commit_done(); }
      if (slot == 5) { transform_finish1(WSC - 1, 4 * (cur ^ 1) * VBUF); raw_load1(WSC - 1); raw_load_done(); }
    } else {
      if (slot == 0) transform_read(4 * (cur ^ 1) * RBUF);
      if (slot == 1) { raw_commit1(0, 4 * cur * RBUF); commit_done(); }
      if (slot == 2) { transform_finish1(0, 4 * (cur ^ 1) * VBUF); raw_load1(0); raw_load_done(); }
    }
  };
  auto side_slice = [&](int slot, int g, int cur) {
    // Every slice runs in every trip (past the end of the stream it works on stale registers and writes LDS buffers nobody
    // reads; the loads stay inside this sample's planes): a slot is then ONE basic block, and the scheduler can place the
    // slice's instructions between the slot's MFMAs (the recipe in the K loop).
    if (WSC == 2) {        // the two chunks' transforms one after the other: their 12 + 12 staging registers are never live together
      // a chunk's raw registers are requested again in the slot right behind their commit: the tile data (HBM) then has seven
      // slots = 7 / 8 of a stage to arrive (both chunks requested together in slot 6 left the first one three slots, ~1.5 us,
      // and its commit waited ~800 cycles for it: in-kernel slot stamps)
      if (slot == 0) transform_read1(0, 4 * (cur ^ 1) * RBUF);
      if (slot == 1) raw_commit1(0, 4 * cur * RBUF);
      if (slot == 2) { transform_finish1(0, 4 * (cur ^ 1) * VBUF); raw_load1(0); }
      if (slot == 3) transform_read1(WSC - 1, 4 * (cur ^ 1) * RBUF);
      if (slot == 4) { raw_commit1(WSC - 1, 4 * cur * RBUF); commit_done(); }
      if (slot == 5) { transform_finish1(WSC - 1, 4 * (cur ^ 1) * VBUF); raw_load1(WSC - 1); raw_load_done(); }
    } else {
      if (slot == 0) transform_read(4 * (cur ^ 1) * RBUF);
      if (slot == 1) { raw_commit1(0, 4 * cur * RBUF); commit_done(); }
      if (slot == 2) { raw_load1(0); raw_load_done(); }
      if (slot == 3) transform_finish1(0, 4 * (cur ^ 1) * VBUF);
    }
  };
  (void)mode;
  int st = 0, tile = tile0;                                        // stage within the tile, tile of the accumulators
  // PAIR: a trip is TWO stages, buffer parity 0 then 1, each with its barrier: the parity is a compile-time constant in either half
  // and with it every LDS offset.  The tile-end check follows the second half only -- the launcher takes this form for even stage
  // counts per tile -- so that the epilogue and init_acc() exist once in the loop.
  for (int g = 0; g < G; g += PAIR ? 2 : 1) {
#pragma unroll
    for (int half = 0; half < (PAIR ? 2 : 1); ++half) {
    const int cur = PAIR ? half : g & 1;
    WINO_STAMP(0)
    WINO_SLOT0
    if constexpr (SPLIT) {
      // SPLIT: a stage is 2 x 4 slots of TWO MFMAs -- k-step s of the wave's two positions, so that every position still sums its
      // chunks ascending, four k-steps per chunk, from the matrix pipe's zero -- and behind each slot the same slice of side work as
      // in the other variants (same slot numbers, one basic block per slot).  The stage's four B fragments are read right behind
      // the barrier, the next stage's four weight fragments requested with them.
      f32x4 bf[WSC][2], wn[WSC][2];
#pragma unroll
      for (int sc = 0; sc < WSC; ++sc) {
        const int vbo = 4 * (cur * VBUF + sc * 16 * VPOS);
        bf[sc][0] = lds_get<f32x4>(vrd, vbo);
        bf[sc][1] = lds_get<f32x4>(vrd, vbo + 4 * VPOS);
      }
#pragma unroll
      for (int sc = 0; sc < WSC; ++sc) {
        const int cn = (st + 1) * WSC + sc;
        wn[sc][0] = wfrag(cn < nch ? cn : 0, 0);
        wn[sc][1] = wfrag(cn < nch ? cn : 0, 1);
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int sc = 0; sc < WSC; ++sc) {
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(wa[sc][0][s], bf[sc][0][s], acc[0], 0, 0, 0);
          acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(wa[sc][1][s], bf[sc][1][s], acc[1], 0, 0, 0);
          side_slice(sc * 4 + s, g, cur);
#pragma unroll
          for (int i = 0; i < 2; ++i) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x486, 4 * WINO_IL_K, 0);       // VALU | SALU | DS | transcendental
          }
          __builtin_amdgcn_sched_group_barrier(0x020, 4, 0);
          __builtin_amdgcn_sched_barrier(0);
          if (sc * 4 + s == 5) raw_load_next();                                   // the one conditional piece (tile geometry): a block of its own
          __builtin_amdgcn_sched_barrier(0);
        }
      }
#pragma unroll
      for (int sc = 0; sc < WSC; ++sc) { wa[sc][0] = wn[sc][0]; wa[sc][1] = wn[sc][1]; }
    } else {
#pragma unroll
    for (int sc = 0; sc < WSC; ++sc) {
      const int c = st * WSC + sc;
      const int cn = c + 1 < nch ? c + 1 : 0;                                 // after a tile's last chunk: chunk 0 again
      const int vbo = 4 * (cur * VBUF + sc * 16 * VPOS);
      if constexpr (UPZ) {
        constexpr int CQ[3] = {0, 1, 3};                   // the blocks both halves run
        f32x4 bq[3];                                       // their B fragments, one position ahead of the MFMAs
        bq[0] = lds_get<f32x4>(vrd, vbo);
        bq[1] = lds_get<f32x4>(vrd, vbo + 4 * VPOS);
        __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          if (i == 0) bq[2] = lds_get<f32x4>(vrd, vbo + 4 * 3 * VPOS);
#pragma unroll
          for (int s = 0; s < 4; ++s) acc[CQ[i]] = __builtin_amdgcn_mfma_f32_32x32x2f32(ua[CQ[i]][s], bq[i][s], acc[CQ[i]], 0, 0, 0);
          if (!no_u) ua[CQ[i]] = wfrag(cn, CQ[i]);
          side_slice_upz(sc * 3 + i, cur);
          if (i == 0) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x486, 2 * WINO_IL_K, 0);
          }
          __builtin_amdgcn_sched_group_barrier(0x020, 4, 0);
          __builtin_amdgcn_sched_barrier(0);
          if (sc * 3 + i == (WSC == 2 ? 5 : 2)) raw_load_next();
          __builtin_amdgcn_sched_barrier(0);
        }
        if (hf == 0) {                                     // xi = 1: blocks 4, 5, 7 (wave-uniform; the hf = 1 waves' xi = 2 is dead)
          constexpr int HQ[3] = {4, 5, 7};
          f32x4 bh[3];
#pragma unroll
          for (int i = 0; i < 3; ++i) bh[i] = lds_get<f32x4>(vrd, vbo + 4 * HQ[i] * VPOS);
#pragma unroll
          for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int s = 0; s < 4; ++s) acc[HQ[i]] = __builtin_amdgcn_mfma_f32_32x32x2f32(ua[HQ[i]][s], bh[i][s], acc[HQ[i]], 0, 0, 0);
            if (!no_u) ua[HQ[i]] = wfrag(cn, HQ[i]);
          }
        }
        __builtin_amdgcn_sched_barrier(0);
      } else {
      f32x4 b4[2][2];                                      // B fragments of two positions, one pair ahead of the MFMAs
      b4[0][0] = lds_get<f32x4>(vrd, vbo);
      b4[0][1] = lds_get<f32x4>(vrd, vbo + 4 * VPOS);
      __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
#pragma unroll
      for (int qp = 0; qp < 4; ++qp) {
        const int cb = qp & 1;
        if (qp < 3) {
          b4[cb ^ 1][0] = lds_get<f32x4>(vrd, vbo + 4 * (2 * qp + 2) * VPOS);
          b4[cb ^ 1][1] = lds_get<f32x4>(vrd, vbo + 4 * (2 * qp + 3) * VPOS);
        }
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          acc[2 * qp] = __builtin_amdgcn_mfma_f32_32x32x2f32(ua[2 * qp][s], b4[cb][0][s], acc[2 * qp], 0, 0, 0);
          acc[2 * qp + 1] = __builtin_amdgcn_mfma_f32_32x32x2f32(ua[2 * qp + 1][s], b4[cb][1][s], acc[2 * qp + 1], 0, 0, 0);
        }
        // the next chunk's weights of these two positions: 2 KB per wave every eight MFMAs.  (All of a chunk's weight loads
        // issued together right behind the barrier -- 64 KB per CU at once -- back up the vector memory path and every
        // wave stalls in their issue for 1000-3000 cycles per chunk.)
        if (!no_u) {
          ua[2 * qp] = wfrag(cn, 2 * qp);
          ua[2 * qp + 1] = wfrag(cn, 2 * qp + 1);
        }
        // The slice's instructions go BETWEEN the slot's MFMAs, up to WINO_IL_K behind each: its dependent chains (LDS read ->
        // arithmetic -> transcendental -> LDS write) then wait under matrix instructions instead of in front of the next slot
        // (as a block of its own behind the eight MFMAs a commit slice cost +900 cycles for ~25 vector instructions).
        side_slice(sc * 4 + qp, g, cur);
        if (qp < 3) __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
          __builtin_amdgcn_sched_group_barrier(0x486, WINO_IL_K, 0);           // VALU | SALU | DS | transcendental
        }
        __builtin_amdgcn_sched_group_barrier(0x020, 4, 0);
        __builtin_amdgcn_sched_barrier(0);
        if (sc * 4 + qp == (WSC == 2 ? 5 : 2)) raw_load_next();                 // the one conditional piece (tile geometry): a block of its own
        __builtin_amdgcn_sched_barrier(0);
        WINO_SLOT(sc * 4 + qp + (WSC == 1 ? 0 : 0))
      }
      }
    }
    }
    WINO_STAMP(1)
    __syncthreads();
    WINO_STAMP(2)
    ++st;
    }
    if (st < nst) continue;
    st = 0;

    // ---- a tile is complete: output transform, bias, residual, stores, statistics; then the accumulators start over.
    // (The stream's LDS buffers already hold the first stages of the next tile: the exchange area is a region of its own.)
    if constexpr (SPLIT) {
      // SPLIT: the workgroup's one tile is complete and its stream has drained (the trip's barrier is behind every wave): the sixteen
      // blocks go to LDS over the V buffers, [position][register][lane].  Then wave (ehf, gq) takes the part of the other variants'
      // wave (mb, hf = ehf) that sits in registers 4 gq .. 4 gq + 3 -- channels 8 gq + 4 (lane >> 5) + {0 .. 3}, patch lane & 31, pixel
      // row ehf -- and evaluates their expressions on it: T_xi over nu, keep + the partner's send over xi, then the residual.
      const int y0 = (tile / tiles_x) * WPH, x0 = (tile % tiles_x) * WPW;
      float* const dump = lds;
#pragma unroll
      for (int q = 0; q < 2; ++q)
#pragma unroll
        for (int r = 0; r < 16; ++r) dump[((2 * wave + q) * 16 + r) * 64 + lane] = acc[q][r];
      const int ehf = wave >> 2, gq = wave & 3, pt = lane & 31;
      const int oy = y0 + 2 * (pt >> 3) + ehf, ox = x0 + 2 * (pt & 7);
      const int cbase = m0 + 8 * gq + 4 * (lane >> 5);
      const size_t splane = (size_t)p.Cout * HW;
      const __amdgpu_buffer_rsrc_t rs_out = make_rsrc(p.out + (size_t)n * splane, 4u * (unsigned)splane);
      const size_t rplane = p.res_mode == RS_DOWN ? splane << 2 : splane;
      const __amdgpu_buffer_rsrc_t rs_res = make_rsrc(p.res ? p.res + (size_t)n * rplane : nullptr, p.res ? 4u * (unsigned)rplane : 0u);
      const unsigned HWu = (unsigned)HW;
      const unsigned voff = 4u * ((unsigned)cbase * HWu + (unsigned)oy * p.W + ox);
      float2 rv[4];
      if (p.res && p.res_mode == RS_DOWN) {               // the 2x2 mean of the source at double resolution, as in the other variants
        const unsigned dvoff = 4u * ((unsigned)cbase * (HWu << 2) + (unsigned)(2 * oy) * (unsigned)(2 * p.W) + (unsigned)(2 * ox));
        f32x4 ta[4], tb[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const unsigned so = 4u * (unsigned)k * (HWu << 2);
          ta[k] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs_res, dvoff, so, 0));
          tb[k] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs_res, dvoff + 8u * (unsigned)p.W, so, 0));
        }
#pragma unroll
        for (int k = 0; k < 4; ++k)
          rv[k] = make_float2(0.25f * ((ta[k][0] + ta[k][1]) + (tb[k][0] + tb[k][1])), 0.25f * ((ta[k][2] + ta[k][3]) + (tb[k][2] + tb[k][3])));
      } else {                                             // no residual: a zero-sized descriptor reads zeros
#pragma unroll
        for (int k = 0; k < 4; ++k) rv[k] = __builtin_bit_cast(float2, __builtin_amdgcn_raw_buffer_load_b64(rs_res, voff, 4u * (unsigned)k * HWu, 0));
      }
      __syncthreads();
      float v0[4], v1[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        // T[i][j]: the nu-reduced block xi = ehf + i for pixel column j (A^T = [[1,1,1,0],[0,1,-1,-1]])
        float T[3][2];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          const float* d = dump + ((4 * (ehf + i)) * 16 + 4 * gq + k) * 64 + lane;
          const float a0 = d[0 * 16 * 64], a1 = d[1 * 16 * 64], a2 = d[2 * 16 * 64], a3 = d[3 * 16 * 64];
          T[i][0] = a0 + a1 + a2;
          T[i][1] = a1 - a2 - a3;
        }
        if (ehf == 0) {                                    // row 0: keep = T0 + T1, the partner sends T2
          v0[k] = (T[0][0] + T[1][0]) + T[2][0] + rv[k].x;
          v1[k] = (T[0][1] + T[1][1]) + T[2][1] + rv[k].y;
        } else {                                           // row 1: keep = -T2 - T3, the partner sends T1
          v0[k] = (-T[1][0] - T[2][0]) + T[0][0] + rv[k].x;
          v1[k] = (-T[1][1] - T[2][1]) + T[0][1] + rv[k].y;
        }
      }
#pragma unroll
      for (int k = 0; k < 4; ++k)
        __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(__attribute__((ext_vector_type(2))) unsigned, make_float2(v0[k], v1[k])), rs_out, voff,
                                              4u * (unsigned)k * HWu, 0);
      if (p.gsum) {                                        // the records of the other variants' wave (mb, hf) for its group gq
        const bool pairs = p.gsum_rc == 2;
        float a[2], b[2];
#pragma unroll
        for (int e = 0; e < 2; ++e) a[e] = half_sum32_swap((v0[2 * e] + v1[2 * e]) + (v0[2 * e + 1] + v1[2 * e + 1]));
        const float cnt = pairs ? 128.f : 256.f;
        const float mean0 = pairs ? a[0] * (1.0f / 128.0f) : (a[0] + a[1]) * (1.0f / 256.0f);
        const float mean1 = pairs ? a[1] * (1.0f / 128.0f) : mean0;
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          const float mean = e ? mean1 : mean0;
          float q = 0.f;
#pragma unroll
          for (int r = 2 * e; r < 2 * e + 2; ++r) { const float d0 = v0[r] - mean, d1 = v1[r] - mean; q = fmaf(d0, d0, q); q = fmaf(d1, d1, q); }
          b[e] = half_sum32_swap(q);
        }
        if ((lane & 31) == 0) {
          const int quad = 2 * gq + (lane >> 5);
          if (pairs) {
#pragma unroll
            for (int e = 0; e < 2; ++e) {
              float* slot = red + (ehf * (C::MT / 2) + 2 * quad + e) * 3;
              slot[0] = cnt; slot[1] = a[e]; slot[2] = b[e];
            }
          } else {
            float* slot = red + (ehf * (C::MT / 4) + quad) * 3;
            slot[0] = cnt; slot[1] = a[0] + a[1]; slot[2] = b[0] + b[1];
          }
        }
        __syncthreads();
        conv_stats_store<C, 2>(p, red, n, m0, tile, tiles_img, tid);
      }
      break;
    }
    WINO_EP(0)
    const int y0 = (tile / tiles_x) * WPH, x0 = (tile % tiles_x) * WPW;
    const int pt = lane & 31;                             // this wave stores row hf of every patch: pixels
    const int oy = y0 + 2 * (pt >> 3) + hf, ox = x0 + 2 * (pt & 7);   // (y0 + 2 ty + hf, x0 + 2 tx + {0, 1}), patch = lane & 31
    const int cbase = m0 + 32 * mb + 4 * (lane >> 5);
    // buffer addressing for the tile's 16 + 16 + 16 memory operations: one descriptor per tensor (this sample's planes) in
    // SGPRs, one 32-bit lane offset, the channel step in the scalar offset -- no 64-bit address pair per operation
    const size_t splane = (size_t)p.Cout * HW;                      // this sample's output planes (the launcher checks < 4 GiB)
    const __amdgpu_buffer_rsrc_t rs_out = make_rsrc(p.out + (size_t)n * splane, 4u * (unsigned)splane);
    const size_t rplane = p.res_mode == RS_UP ? splane >> 2 : p.res_mode == RS_DOWN ? splane << 2 : splane;   // the residual's planes of this sample
    const __amdgpu_buffer_rsrc_t rs_res = make_rsrc(p.res ? p.res + (size_t)n * rplane : nullptr, p.res ? 4u * (unsigned)rplane : 0u);
    const unsigned HWu = (unsigned)HW;
    const unsigned voff = 4u * ((unsigned)cbase * HWu + (unsigned)oy * p.W + ox);
    const unsigned rvoff = 4u * ((unsigned)cbase * (HWu >> 2) + (unsigned)(oy >> 1) * (p.W >> 1) + (ox >> 1));
    // A^T = [[1,1,1,0],[0,1,-1,-1]].  Over nu (register-local), then over xi across the two halves: row 0 of the patch =
    // T0 + T1 + T2, row 1 = T1 - T2 - T3 with T_xi the nu-reduced blocks; half 0 holds T0, T1, half 1 T2, T3.
    f32x16 keep[2], send[2];
    float v0[16], v1[16];
    SkipFold<C> sk;                                       // SKIP: the projection's first operands are requested here, under the transform
    if constexpr (SKIP) sk.begin(p, skbuf, n, m0 / 32 + mb, mblocks, y0, x0, tid, lane, hf);
#pragma unroll
    for (int j = 0; j < 2; ++j) {                          // one pixel column at a time: fewer values live beside the accumulators
      const f32x16 t0 = j == 0 ? acc[0] + acc[1] + acc[2] : acc[1] - acc[2] - acc[3];
      const f32x16 t1 = j == 0 ? acc[4] + acc[5] + acc[6] : acc[5] - acc[6] - acc[7];
      // UPZ: the hf = 1 waves hold T3 in blocks 0 .. 3 (t0) and the dead T2 = +0 in blocks 4 .. 7 (t1): same expressions, roles swapped
      if (hf == 0)  { keep[j] = t0 + t1; send[j] = t1; }
      else if (UPZ) { keep[j] = -t1 - t0; send[j] = t1; }
      else          { keep[j] = -t0 - t1; send[j] = t0; }
      __builtin_amdgcn_sched_barrier(0);
    }
    // (chunk 0's weights for the next tile came with the stream's reload at this tile's last chunk.  Fetching them AGAIN here --
    // to end the first copy's life at the last MFMA -- was round 3's way to 32 free registers during the transform; without it the
    // kernel spills 3 registers instead of 7, issues 64 fewer vector-memory instructions per tile and CU, and is 0.4 % faster.
    // Exchanging the halves through 16-byte LDS accesses, lane pitch 20 floats, measured 1.5 % slower at 128 channels.)
    __builtin_amdgcn_sched_barrier(0);                    // the accumulators are dead from here to the end of the epilogue
    if constexpr (SKIP) {
      WINO_EP(1)                                          // 1: output transform over nu, first projection requests
      sk.run(xch, skb_l + 32 * mb + 4 * (lane >> 5), wave, wave ^ MB, lane, keep, send, v0, v1);
      WINO_EP(2)                                          // 2: the projection with the two exchange rounds inside it
    } else {
    // residual: in flight during the rest of the transform and the exchange.  ONE wave-uniform dispatch on its mode, every arm
    // straight-line: rx / ry = what is added to the left / right pixel of the pair; nothing behind the arms knows the mode.
    // RS_UP: both pixels share a source, and each asks for it with a load of its own -- a copy behind the load (rx = ry = q) had put
    // a wait for the whole round trip between every two loads; one register for both, added where v1 is formed, lives through both
    // exchange rounds and costs every instantiation spills.  The second load hits the line the first fetched.
    float rx[16], ry[16];
    const int rmode = p.res ? p.res_mode : RS_NONE;
    if (rmode == RS_DOWN) {
      // residual at double resolution: the 2x2 mean of the source (adm_blocks.py:75-77), two 16-byte loads per channel and
      // pixel pair, four channels in flight at a time.  (Eight, as a rolling window -- the accumulators are dead here -- spill nothing
      // and change nothing: the tile's 256 KB per CU arrive at the rate the memory system has for them)
      const unsigned dvoff = 4u * ((unsigned)cbase * (HWu << 2) + (unsigned)(2 * oy) * (unsigned)(2 * p.W) + (unsigned)(2 * ox));
#pragma unroll
      for (int r0 = 0; r0 < 16; r0 += 4) {
        f32x4 ta[4], tb[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const unsigned so = 4u * (unsigned)(((r0 + k) & 3) + 8 * ((r0 + k) >> 2)) * (HWu << 2);
          ta[k] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs_res, dvoff, so, 0));
          tb[k] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs_res, dvoff + 8u * (unsigned)p.W, so, 0));
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          rx[r0 + k] = 0.25f * ((ta[k][0] + ta[k][1]) + (tb[k][0] + tb[k][1]));
          ry[r0 + k] = 0.25f * ((ta[k][2] + ta[k][3]) + (tb[k][2] + tb[k][3]));
        }
      }
    } else if (rmode == RS_UP) {                           // residual at half resolution: 2 x 16 loads back to back, no copy, no wait
#pragma unroll
      for (int r = 0; r < 16; ++r)
        rx[r] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs_res, rvoff, 4u * (unsigned)((r & 3) + 8 * (r >> 2)) * (HWu >> 2), 0));
      unsigned rvoff_y = rvoff;                            // opaque: or the two loads of a channel become one and the copy is back
      asm volatile("" : "+v"(rvoff_y));
#pragma unroll
      for (int r = 0; r < 16; ++r)
        ry[r] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs_res, rvoff_y, 4u * (unsigned)((r & 3) + 8 * (r >> 2)) * (HWu >> 2), 0));
    } else {                                               // same resolution; no residual: a zero-sized descriptor reads zeros
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float2 q = __builtin_bit_cast(float2, __builtin_amdgcn_raw_buffer_load_b64(rs_res, voff, 4u * (unsigned)((r & 3) + 8 * (r >> 2)) * HWu, 0));
        rx[r] = q.x; ry[r] = q.y;
      }
    }
    WINO_EP(1)                                            // 1: output transform over nu, weight + residual requests
    const int pw = wave ^ MB;
#pragma unroll
    for (int j = 0; j < 2; ++j) {                         // two rounds of 16 registers through the exchange area
#pragma unroll
      for (int r = 0; r < 16; ++r) xch[(wave * 16 + r) * 64 + lane] = send[j][r];
      __syncthreads();
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float got = xch[(pw * 16 + r) * 64 + lane];
        if (j == 0) v0[r] = keep[0][r] + got + rx[r];
        else        v1[r] = keep[1][r] + got;
      }
      if (j == 0) __syncthreads();
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) v1[r] = v1[r] + ry[r];     // (keep + got) + residual, as for v0
    WINO_EP(2)                                            // 2: the two exchange rounds (incl. the wait for the residual)
    }
#pragma unroll
    for (int r = 0; r < 16; ++r)
      __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(__attribute__((ext_vector_type(2))) unsigned, make_float2(v0[r], v1[r])), rs_out, voff,
                                            4u * (unsigned)((r & 3) + 8 * (r >> 2)) * HWu, 0);
    WINO_EP(3)                                            // 3: the 16 stores
    if (p.gsum) {
      // fused GroupNorm statistics of what was stored (conv_tile.hpp conv_epilogue): one record per 4-channel block =
      // registers 4 g .. 4 g + 3 of the 32 lanes that share lane >> 5 (or per 2-channel block, gsum_rc == 2: their two
      // halves); this wave holds one pixel row of every patch, its partner wave the other: (count, sum, M2 about the wave's
      // own mean) per wave, merged in a fixed order by conv_stats_store.
      // The record width is tested ONCE, in front of the four groups, and the slots in `red` are addressed from an opaque copy of
      // the thread index: nothing of this phase is computed ahead of the K loop and kept (or spilled) through it.
      int ol = tid;
      asm volatile("" : "+v"(ol));
      const int half = (ol >> 5) & 1;
      const bool first = (ol & 31) == 0;
      auto stats = [&](auto PAIRS) {
        constexpr bool pairs = decltype(PAIRS)::value;
        constexpr float cnt = pairs ? 128.f : 256.f;
        float* const slot0 = red + (pairs ? hf * (C::MT / 2) + 2 * (8 * mb + half) : hf * (C::MT / 4) + 8 * mb + half) * 3;
#pragma unroll
        for (int gq = 0; gq < 4; ++gq) {
          float a[2], b[2];
#pragma unroll
          for (int e = 0; e < 2; ++e) {
            a[e] = half_sum32_swap((v0[4 * gq + 2 * e] + v1[4 * gq + 2 * e]) + (v0[4 * gq + 2 * e + 1] + v1[4 * gq + 2 * e + 1]));
          }
          const float mean0 = pairs ? a[0] * (1.0f / 128.0f) : (a[0] + a[1]) * (1.0f / 256.0f);
          const float mean1 = pairs ? a[1] * (1.0f / 128.0f) : mean0;
#pragma unroll
          for (int e = 0; e < 2; ++e) {
            const float mean = e ? mean1 : mean0;
            float q = 0.f;
#pragma unroll
            for (int r = 4 * gq + 2 * e; r < 4 * gq + 2 * e + 2; ++r) { const float d0 = v0[r] - mean, d1 = v1[r] - mean; q = fmaf(d0, d0, q); q = fmaf(d1, d1, q); }
            b[e] = half_sum32_swap(q);
          }
          if (first) {                                     // quad = 8 mb + 2 gq + half: slot 2 quad + e (pairs) or quad
            if constexpr (pairs) {
#pragma unroll
              for (int e = 0; e < 2; ++e) {
                float* slot = slot0 + (4 * gq + e) * 3;
                slot[0] = cnt; slot[1] = a[e]; slot[2] = b[e];
              }
            } else {
              float* slot = slot0 + 2 * gq * 3;
              slot[0] = cnt; slot[1] = a[0] + a[1]; slot[2] = b[0] + b[1];
            }
          }
        }
      };
      if (p.gsum_rc == 2) stats(std::true_type{}); else stats(std::false_type{});
      __syncthreads();
      conv_stats_store<C, 2>(p, red, n, m0, tile, tiles_img, tid);
      // the next epilogue writes `red` only after a whole tile of barriers
    }
    WINO_EP(4)                                            // 4: statistics
    __builtin_amdgcn_sched_barrier(0);
    init_acc();
    tile += tstep;
    WINO_EP(5)                                            // 5: accumulator initialisation
    WINO_STAMP(3)
  }
  if (p.dbg && tid == 0) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    p.dbg[blockIdx.x * 16 + 2] = __builtin_amdgcn_s_memrealtime(); p.dbg[blockIdx.x * 16 + 6] = __builtin_amdgcn_s_memtime();
    p.dbg[blockIdx.x * 16 + 3] = __builtin_amdgcn_s_memrealtime();
  }
#ifdef MCEDM_WINO_TIMELINE
  if (p.dbg && tid == 0) for (int i = 0; i < 5; ++i) p.dbg[blockIdx.x * 16 + 8 + i] = ph[i];
  if (p.dbg && tid == 0 && (mode & 16)) for (int i = 0; i < 8; ++i) p.dbg[blockIdx.x * 16 + 8 + i] = sl[i];
  if (p.dbg && tid == 0 && (mode & 32)) for (int i = 0; i < 6; ++i) p.dbg[blockIdx.x * 16 + 8 + i] = ep[i];
  if (p.dbg && tid == 64 * MB && !(mode & 48)) { p.dbg[blockIdx.x * 16 + 13] = ph[1]; p.dbg[blockIdx.x * 16 + 14] = ph[2]; p.dbg[blockIdx.x * 16 + 15] = ph[3]; p.dbg[blockIdx.x * 16 + 7] = ph[0]; }
#endif
}

// The switches of this file (switches.hpp) -- KV_CONV_WINO = 0: never take this kernel; KV_CONV_WINO_FOLD = 0: the skip projection stays
// a launch of its own; KV_CONV_WINO_UPZ = 0: the up-sampling convs run all sixteen positions; KV_CONV_WINO_SPLIT = 0: the small images'
// 3x3 convs stay on the input-resident / tiled kernels.
static int wino_mode_env() {                                  // MCEDM_WINO_MODE: ablation bits of the -DMCEDM_WINO_TIMELINE build (else unused)
  static const int env =                                       // | 256: the interleaved, XCD-aware tile map (MCEDM_WINO_MAP, default on)
      (env_int("MCEDM_WINO_MODE", 0) & ~256) | (env_int("MCEDM_WINO_MAP", 1) ? 256 : 0);
  return env;
}

static int wino_min_hw_env() {                                 // MCEDM_WINO_MIN_HW: smallest image (pixels) served; below 32 x 32 the grid
  static const int env = env_int("MCEDM_WINO_MIN_HW", 1024);   // (B * H * W / 128 workgroups) no longer fills the chip
  return env;
}

size_t conv_frag_packed_floats(int Cout, int Cin) { return (size_t)cout_padded(Cout) * (size_t)ceil_div(Cin, 8) * 8; }

int launch_pack_conv_frag(const float* w, float* dst, int Cout, int Cin, hipStream_t stream) {
  MCEDM_REQUIRE(w && dst && Cout > 0 && Cin > 0, "pack_conv_frag: bad arguments");
  const int coutp = cout_padded(Cout), cinp = ceil_div(Cin, 8) * 8;
  hipLaunchKernelGGL(conv_frag_pack_kernel, dim3(ceil_div(coutp * cinp, 256)), dim3(256), 0, stream, w, dst, Cout, Cin, coutp, cinp);
  MCEDM_LAUNCH_CHECK("conv_frag_pack_kernel");
  return MCEDM_OK;
}

size_t conv_wino_packed_floats(int Cout, int Cin) { return (size_t)16 * cout_padded(Cout) * (size_t)ceil_div(Cin, WKC) * WKC; }

int launch_pack_conv_wino(const float* w, float* dst, int Cout, int Cin, int transpose_flip, hipStream_t stream) {
  MCEDM_REQUIRE(w && dst && Cout > 0 && Cin > 0, "pack_conv_wino: bad arguments");
  const int coutp = cout_padded(Cout), nch = ceil_div(Cin, WKC);
  hipLaunchKernelGGL(wino_pack_kernel, dim3(ceil_div(coutp * nch * WKC, 256)), dim3(256), 0, stream, w, dst, Cout, Cin, coutp, nch,
                     transpose_flip);
  MCEDM_LAUNCH_CHECK("wino_pack_kernel");
  return MCEDM_OK;
}

// A folded 1x1 projection (ConvArgs::sk_*) is served by the SKIP variant of the plain, activated, 128-channel kernel: whole stages
// of 16 channels out of either source (at least two: the exchange rounds ride on the first two stage barriers), 16-byte loads,
// one sample of each source below the 4 GiB range of its buffer descriptor.
static bool conv_wino_fold_ok(const ConvArgs& a) {
  const int Csk = a.sk_Ca + a.sk_Cb;
  const unsigned long long HW = (unsigned long long)a.H * a.W;
  return kernel_switch(KV_CONV_WINO_FOLD) != 0 && a.sk_wfrag && a.resample == RS_NONE && !a.res && a.act && a.Cout % 128 == 0 && a.sk_xa && a.sk_Ca > 0 &&
         a.sk_Cb >= 0 && (a.sk_Cb > 0) == (a.sk_xb != nullptr) && a.sk_Ca % 16 == 0 && a.sk_Cb % 16 == 0 && Csk >= 32 && Csk <= 256 &&
         (((size_t)a.sk_xa | (size_t)a.sk_xb | (size_t)a.sk_wfrag) & 15) == 0 && HW * 4ull * (unsigned long long)a.sk_Ca < (1ull << 32) &&
         HW * 4ull * (unsigned long long)a.sk_Cb < (1ull << 32);
}
// plan-time question (build_layout): will conv1 of an un-resampled block (Csk -> Cout skip projection) take the fold?
bool conv_wino_fold_shape_ok(int Cout, int sk_Ca, int sk_Cb, int H, int W) {
  const int Csk = sk_Ca + sk_Cb;
  return kernel_switch(KV_CONV_WINO_FOLD) != 0 && conv_wino_shape_ok(Cout, Cout, H, W) && Cout % 128 == 0 && sk_Ca > 0 && sk_Ca % 16 == 0 && sk_Cb % 16 == 0 &&
         Csk >= 32 && Csk <= 256 && (unsigned long long)H * W * 4ull * (unsigned long long)(sk_Ca > sk_Cb ? sk_Ca : sk_Cb) < (1ull << 32);
}

bool conv_wino_applicable(const ConvArgs& a, int taps) {
  // the plain variant stages its input with 16-byte loads (raw_load1): misaligned views take the direct kernel
  const bool aligned = a.resample != RS_NONE || (((size_t)a.xa | (size_t)a.xb) & 15) == 0;
  return taps == 9 && a.wino && (a.resample == RS_NONE || a.resample == RS_UP) && a.Cout % 64 == 0 && a.H % WPH == 0 && aligned &&
         a.W % WPW == 0 && (a.Ca + a.Cb) % WKC == 0 && a.Ca % WKC == 0 && (!a.sk_wpk || conv_wino_fold_ok(a)) && ((size_t)a.wino & 15) == 0 &&
         (!a.res || a.res_mode == RS_NONE || a.res_mode == RS_UP || a.res_mode == RS_DOWN) && (a.Ca + a.Cb) <= 1024;
}

// Tiles per workgroup: a divisor d of the tiles per image (a workgroup stays inside one sample: one set of transform rows),
// chosen for the shortest schedule on `slots` concurrent workgroups -- rounds x (d tiles + the un-overlapped start and end
// of a workgroup, about a fifth of a tile).  A function of the shape and the chip only: results never depend on it.
int wino_tiles_per_wg(long long total, int tiles_img, int slots) {
  int best = 1;
  double best_t = 1e30;
  for (int d = 1; d <= tiles_img; ++d) {
    if (tiles_img % d) continue;
    const long long wgs = total / d;
    const double t = (double)((wgs + slots - 1) / slots) * (d + 0.2);
    if (t < best_t - 1e-9 || (t < best_t + 1e-9 && d > best)) { best_t = t; best = d; }
  }
  return best;
}

// The two forms of every instantiation (conv_wino.hpp WinoLoop1): the two-stage trip with immediate LDS offsets and buffer descriptors
// serves the launches whose tiles have an EVEN number of stages (it ends a tile behind the second stage of a trip only) and whose
// Winograd table lies inside a descriptor's 4 GiB range; everything else keeps the one-stage trip.  Three instantiations stay on the
// one-stage trip for every shape, because hipcc spills more in the two-stage form than their present code does:
// the sixteen-position up-sampling kernels (KV_CONV_WINO_UPZ = 0) and the 64-channel kernel without activation.
template <class C, bool UP, bool ACT, class... Tag>
constexpr bool wino_pair_form = !(UP && sizeof...(Tag) == 0) && !(C::MB == 2 && !UP && !ACT);
static bool wino_loop1(const ConvArgs& a, int chunks_per_stage) {
  const unsigned long long Cin = (unsigned long long)(a.Ca + a.Cb);
  const int nst = ceil_div((int)Cin / WKC, chunks_per_stage);
  const unsigned long long table = 16ull * Cin * (unsigned long long)cout_padded(a.Cout) * 4ull;
  return nst % 2 != 0 || table >= (1ull << 32);
}
template <class C, bool UP, bool ACT, class... Tag>
static void wino_launch(bool loop1, dim3 grid, int lds_bytes, hipStream_t stream, const ConvArgs& a, int tiles_x, int tiles_img, int nch, int mblocks, int per,
                        int mode) {
  if constexpr (wino_pair_form<C, UP, ACT, Tag...>) {
    if (!loop1) {
      hipLaunchKernelGGL((conv_wino_kernel<C, UP, ACT, Tag...>), grid, dim3(C::NT), lds_bytes, stream, a, tiles_x, tiles_img, nch, mblocks, per, mode);
      return;
    }
  }
  hipLaunchKernelGGL((conv_wino_kernel<C, UP, ACT, WinoLoop1, Tag...>), grid, dim3(C::NT), lds_bytes, stream, a, tiles_x, tiles_img, nch, mblocks, per, mode);
}
template <class C, bool UP, bool ACT, class... Tag>
static hipError_t wino_lds_attr() {
  if constexpr (wino_pair_form<C, UP, ACT, Tag...>) {
    const hipError_t e = hipFuncSetAttribute((const void*)conv_wino_kernel<C, UP, ACT, Tag...>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) return e;
  }
  return hipFuncSetAttribute((const void*)conv_wino_kernel<C, UP, ACT, WinoLoop1, Tag...>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
}

template <class C>
static int launch_wino_cfg(const ConvArgs& a, hipStream_t stream) {
  const int tiles_x = a.W / WPW, tiles_img = tiles_x * (a.H / WPH);
  const long long total = (long long)a.B * tiles_img;
  MCEDM_REQUIRE(total > 0 && total <= 0x7fffffffLL, "conv_wino: grid out of range");
  const int Cin = a.Ca + a.Cb, nch = Cin / WKC;
  int sk_floats = 0;
  if constexpr (C::SKIP) sk_floats = C::SK_FLOATS;
  const int lds_bytes = (C::LDS_ROWS_OFF + 4 * Cin + C::XCH_FLOATS + C::RED_FLOATS + sk_floats) * 4;
  MCEDM_REQUIRE(lds_bytes <= 160 * 1024 / (C::MB == 4 ? 1 : 2), "conv_wino: %d input channels exceed the LDS row table", Cin);
  static std::atomic<bool> attr_set[64];
  static std::atomic<int> ncu[64];
  int dev = 0;
  MCEDM_HIP_TRY(hipGetDevice(&dev));
  MCEDM_REQUIRE(dev >= 0 && dev < 64, "device index %d out of range", dev);
  if (!attr_set[dev].load(std::memory_order_acquire)) {
    int n_cu = 0;
    MCEDM_HIP_TRY(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev));
    ncu[dev].store(n_cu > 0 ? n_cu : 256, std::memory_order_release);
    MCEDM_HIP_TRY((wino_lds_attr<C, false, true>()));
    if constexpr (!C::SKIP) {                              // the SKIP variant exists in the plain, activated form only
      MCEDM_HIP_TRY((wino_lds_attr<C, true, true>()));
      MCEDM_HIP_TRY((wino_lds_attr<C, true, true, WinoUp<true>>()));
      MCEDM_HIP_TRY((wino_lds_attr<C, true, true, WinoUp<false>>()));
      MCEDM_HIP_TRY((wino_lds_attr<C, false, false>()));
      MCEDM_HIP_TRY((wino_lds_attr<C, false, true, WinoBiasRows>()));
    }
    attr_set[dev].store(true, std::memory_order_release);
  }
  const int per_env = wino_per_env();
  int per = wino_tiles_per_wg(total, tiles_img, ncu[dev].load(std::memory_order_acquire) * (C::MB == 4 ? 1 : 2));
  if (per_env > 0 && tiles_img % per_env == 0) per = per_env;
  char name[64] = "";
  const bool noact = a.resample != RS_UP && !a.act;
  // a bias row per sample: the un-resampled, activated kernel alone has that form (the DDPM U-Net's conv1)
  MCEDM_REQUIRE(a.bias_batch == 0 || (!C::SKIP && a.resample == RS_NONE && a.act && a.bias),
                "conv_wino: a bias row per sample (bias_batch=%d) goes with an un-resampled, activated conv without a folded projection", a.bias_batch);
  // the zero-position variant (WinoUp: same LDS footprint); 2: with the sixteen-position kernel's staging (the positions alone, A/B runs)
  const int upz = !C::SKIP && a.resample == RS_UP ? kernel_switch(KV_CONV_WINO_UPZ) : 0;
  if (prof_enabled()) snprintf(name, sizeof(name), "conv_wino_kernel<Wino%sCfg<%d>, %s, %s%s>", C::SKIP ? "Skip" : "", C::MB, a.resample == RS_UP ? "true" : "false",
                               noact ? "false" : "true", a.bias_batch ? ", WinoBiasRows" : upz == 2 ? ", WinoUp<false>" : upz ? ", WinoUp<true>" : "");   // = rocprofv3's name (less the WinoLoop1 tag of the one-stage form)
  const double px = (double)a.B * a.H * a.W;
  const double skc = C::SKIP ? (double)(a.sk_Ca + a.sk_Cb) : 0.0;      // folded 1x1 projection: its own flops, input read and weights
  // algorithmic cost = the direct convolution's (2 * MAC); the kernel issues 4 / 9 of these as matrix flops
  ProfScope ps(name, 2.0 * px * a.Cout * ((double)Cin * 9 + skc),
               4.0 * ((double)a.B * Cin * a.Hs * a.Ws + px * (a.Cout * (a.res ? 2 : 1) + skc) + (double)a.Cout * (Cin * 9 + skc)), stream);
  const dim3 grid((unsigned)(total / per), a.Cout / C::MT);
  const int mblocks = cout_padded(a.Cout) / 32, mode = wino_mode_env();
  const bool loop1 = wino_loop1(a, C::SC);
  if constexpr (C::SKIP)
    wino_launch<C, false, true>(loop1, grid, lds_bytes, stream, a, tiles_x, tiles_img, nch, mblocks, per, mode);
  else if (a.bias_batch)
    wino_launch<C, false, true, WinoBiasRows>(loop1, grid, lds_bytes, stream, a, tiles_x, tiles_img, nch, mblocks, per, mode);
  else if (upz == 2)
    wino_launch<C, true, true, WinoUp<false>>(loop1, grid, lds_bytes, stream, a, tiles_x, tiles_img, nch, mblocks, per, mode);
  else if (upz)
    wino_launch<C, true, true, WinoUp<true>>(loop1, grid, lds_bytes, stream, a, tiles_x, tiles_img, nch, mblocks, per, mode);
  else if (a.resample == RS_UP)
    wino_launch<C, true, true>(loop1, grid, lds_bytes, stream, a, tiles_x, tiles_img, nch, mblocks, per, mode);
  else if (noact)
    wino_launch<C, false, false>(loop1, grid, lds_bytes, stream, a, tiles_x, tiles_img, nch, mblocks, per, mode);
  else
    wino_launch<C, false, true>(loop1, grid, lds_bytes, stream, a, tiles_x, tiles_img, nch, mblocks, per, mode);
  MCEDM_LAUNCH_CHECK("conv_wino_kernel");
  if (a.gsum_tiles) *a.gsum_tiles = SumTiles{tiles_img, tiles_x, WPH, WPW, a.gsum_rc == 2 ? 2 : 4};
  return MCEDM_OK;
}

int launch_conv_wino(const ConvArgs& a_in, hipStream_t stream) {
  ConvArgs a = a_in;
  a.dbg = conv_debug_buffer();
  MCEDM_REQUIRE(conv_wino_applicable(a, 9), "conv_wino: shape not served by the Winograd kernel");
  MCEDM_REQUIRE(a.out && a.B > 0 && (a.resample == RS_UP ? (a.Hs * 2 == a.H && a.Ws * 2 == a.W) : (a.Hs == a.H && a.Ws == a.W)),
                "conv_wino: bad arguments");
  MCEDM_REQUIRE((unsigned long long)a.H * a.W * 4ull * a.Cout * (a.res && a.res_mode == RS_DOWN ? 4 : 1) < (1ull << 32),
                "conv_wino: one sample of the output / residual exceeds the 4 GiB buffer range");
  { const int rc = conv_resolve_identity(a); if (rc != MCEDM_OK) return rc; }
  // 128 output channels per workgroup where they divide (fewer passes over the input), else 64; the 128-channel shape runs on
  // the one-wave-per-SIMD kernel (conv_wino1.hip) only when that is switched on (MCEDM_WINO1=1; off by default)
  if (a.sk_wpk) return launch_wino_cfg<WinoSkipCfg<4>>(a, stream);      // the SKIP variant (conv_wino_fold_ok); never the one-wave kernel
  if (a.Cout % 128 == 0 && !a.bias_batch) {      // (the one-wave kernel has no form with a bias row per sample)
    const int rc = try_launch_conv_wino1(a, stream);
    if (rc != -1) return rc;
  }
  return a.Cout % 128 == 0 ? launch_wino_cfg<WinoCfg<4>>(a, stream) : launch_wino_cfg<WinoCfg<2>>(a, stream);
}

// plan-time question (build_layout): will an un-resampled Cin -> Cout conv on H x W images be served here?
bool conv_wino_shape_ok(int Cout, int Cin, int H, int W) {
  return kernel_switch(KV_CONV_WINO) != 0 && Cout % 64 == 0 && Cin % WKC == 0 && H % WPH == 0 && W % WPW == 0 && (long long)H * W >= wino_min_hw_env();
}
// the dispatcher's choice: enabled, and an image large enough for the grid to fill the chip
bool conv_wino_preferred(const ConvArgs& a) { return kernel_switch(KV_CONV_WINO) != 0 && (long long)a.H * a.W >= wino_min_hw_env(); }

// ---- the SPLIT variant (WinoSplitCfg): the images below that size
bool conv_wino_small(int H, int W) { return (long long)H * W < wino_min_hw_env(); }
bool conv_wino_split_preferred() { return kernel_switch(KV_CONV_WINO) != 0 && kernel_switch(KV_CONV_WINO_SPLIT) != 0; }
// Un-resampled 3x3 convs with a Winograd table on whole 8 x 16 tiles, whole 32-channel output blocks and whole chunks out of either
// source; residual absent, same-size or the 2x2 mean of a double-resolution source.  A folded skip projection, a bias row per
// sample and anything misaligned stay with the direct kernels.
bool conv_wino_split_applicable(const ConvArgs& a, int taps) {
  const int Cin = a.Ca + a.Cb;
  return taps == 9 && a.wino && a.resample == RS_NONE && !a.sk_wpk && a.bias_batch == 0 && conv_wino_small(a.H, a.W) && a.Cout % 32 == 0 &&
         a.H % WPH == 0 && a.W % WPW == 0 && a.Ca > 0 && a.Cb >= 0 && Cin % WKC == 0 && a.Ca % WKC == 0 && Cin <= 1024 &&
         (((size_t)a.xa | (size_t)a.xb | (size_t)a.wino) & 15) == 0 && (!a.res || a.res_mode == RS_NONE || a.res_mode == RS_DOWN);
}

int launch_conv_wino_split(const ConvArgs& a_in, hipStream_t stream) {
  typedef WinoSplitCfg C;
  ConvArgs a = a_in;
  a.dbg = nullptr;                                         // the in-kernel stamps are the large kernels'
  MCEDM_REQUIRE(conv_wino_split_applicable(a, 9), "conv_wino_split: shape not served by the split Winograd kernel");
  MCEDM_REQUIRE(a.out && a.B > 0 && a.Hs == a.H && a.Ws == a.W, "conv_wino_split: bad arguments");
  MCEDM_REQUIRE((unsigned long long)a.H * a.W * 4ull * a.Cout * (a.res && a.res_mode == RS_DOWN ? 4 : 1) < (1ull << 32),
                "conv_wino_split: one sample of the output / residual exceeds the 4 GiB buffer range");
  { const int rc = conv_resolve_identity(a); if (rc != MCEDM_OK) return rc; }
  const int tiles_x = a.W / WPW, tiles_img = tiles_x * (a.H / WPH), nmb = a.Cout / C::MT;
  const long long total = (long long)a.B * tiles_img * nmb;
  MCEDM_REQUIRE(total > 0 && total <= 0x7fffffffLL, "conv_wino_split: grid out of range");
  const int Cin = a.Ca + a.Cb, nch = Cin / WKC;
  const int lds_bytes = (C::LDS_ROWS_OFF + 4 * Cin + C::XCH_FLOATS + C::RED_FLOATS) * 4;
  MCEDM_REQUIRE(lds_bytes <= 160 * 1024, "conv_wino_split: %d input channels exceed the LDS row table", Cin);
  static std::atomic<bool> attr_set[64];
  int dev = 0;
  MCEDM_HIP_TRY(hipGetDevice(&dev));
  MCEDM_REQUIRE(dev >= 0 && dev < 64, "device index %d out of range", dev);
  if (!attr_set[dev].load(std::memory_order_acquire)) {
    MCEDM_HIP_TRY((wino_lds_attr<C, false, true>()));
    MCEDM_HIP_TRY((wino_lds_attr<C, false, false>()));
    attr_set[dev].store(true, std::memory_order_release);
  }
  char name[64] = "";
  if (prof_enabled()) snprintf(name, sizeof(name), "conv_wino_kernel<WinoSplitCfg, false, %s>", a.act ? "true" : "false");   // = rocprofv3's name
  const double px = (double)a.B * a.H * a.W;
  ProfScope ps(name, 2.0 * px * a.Cout * (double)Cin * 9,
               4.0 * ((double)a.B * Cin * a.H * a.W + px * a.Cout * (a.res ? 2 : 1) + (double)a.Cout * Cin * 9), stream);
  const bool loop1 = wino_loop1(a, C::SC);
  if (a.act)
    wino_launch<C, false, true>(loop1, dim3((unsigned)total), lds_bytes, stream, a, tiles_x, tiles_img, nch, cout_padded(a.Cout) / 32, 1, 0);
  else
    wino_launch<C, false, false>(loop1, dim3((unsigned)total), lds_bytes, stream, a, tiles_x, tiles_img, nch, cout_padded(a.Cout) / 32, 1, 0);
  MCEDM_LAUNCH_CHECK("conv_wino_kernel");
  if (a.gsum_tiles) *a.gsum_tiles = SumTiles{tiles_img, tiles_x, WPH, WPW, a.gsum_rc == 2 ? 2 : 4};
  return MCEDM_OK;
}

}  // namespace mcedm
