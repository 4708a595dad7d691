// ---------------------------------------------------------------------------------------------------------
// conv_block_kernel: a whole stride-1 identity bottleneck (nn.py:503-521) in one launch, fp16x2 arithmetic
// (conv_split_common.hpp):  out = relu(conv3(relu(conv2(relu(conv1(x))))) + x),  conv1 1x1 4C -> C, conv2 3x3 C -> C,
// conv3 1x1 C -> 4C, BN folded, C = 64 (res2).  The two launches it replaces (conv_h2_kernel for conv1, conv_h2k_kernel<1,
// false, true> for conv2 + conv3) write conv1's [M, 64] tensor, read it back with a halo and read x a second time as the
// shortcut; here x is read once from HBM (the shortcut read hits the lines phase 1 has just pulled through L2).
// One workgroup of eight waves per 16 x 16 output pixels of one image, three phases:
//   1. conv1 on the tile's 18 x 18 pixel patch (324 rows, padded to 12 MFMA row blocks = 384): a [384 x 256] . [256 x 64] GEMM
//      in conv_h2_kernel's loop form -- BK = 32 stages, x: f32 -> registers (one stage ahead) -> x 2^s (the tensor's recorded
//      |max|) -> hi / lo -> LDS, weights by LDS-DMA, two stages of each.  Operands swapped (lanes along the pixels, registers
//      along the channels); wave w owns row blocks 3 (w / 2) .. + 2 of channel half w % 2 (48 accumulator registers).
//      Epilogue in registers: relu(acc 2^-s 2^-t_c + bias_c); patch pixels OUTSIDE the image become zero (conv2 pads conv1's
//      output with zeros, not with relu(bias)); ONE power of two per tile from the patch's |max| (one workgroup reduction);
//      the pieces go once into the patch image [piece 2][k-group 8][row 384][8 f16], whose k order is the accumulators'
//      register order (conv2's weight image carries the same permutation: conv_make_h2p_weights).  The image takes the place
//      of the A / W stages, which are dead by then.
//   2. conv2 from the patch: 18 stages (32-channel slice x 9 taps); the A fragment of (pixel, tap) is 16 bytes at the lane's
//      base + a compile-time constant (conv_stem_kernel's scheme: no global loads, no splits, no LDS stores in the loop); the
//      weights come through a four-deep LDS-DMA ring, three stages ahead.  Waves 4 x 2 over [256 pixels] x [64 channels],
//      operands swapped: acc[2][1] is exactly what h2f_tail<1> takes.
//   3. conv3 + shortcut + ReLU + store + |max|: h2f_tail<1> (conv_h2f_tail.hpp) over the dead patch, with the rows of the
//      16 x 16 tile in place of 256 consecutive pixels.
// LDS: phase 1 2 x 49 408 (A) + 2 x 8 192 (W) = 115 200 B; phase 2 98 304 (patch) + 4 x 8 192 (ring) = 131 072 B; phase 3 the
// tail's 100 352 B; + 256 B for the reduction = 131 328 B, one workgroup per CU.
// Reference ops: as conv_split.hip.
#include <atomic>
#include "conv_h2f_tail.hpp"

namespace odt {

namespace {

template <int C>
struct BlockCfg {
  static_assert(C == 64, "conv_block_kernel: C = 64 (a 128-wide block needs an 8 x 16 tile and a 128-row tail)");
  using T = H2kCfg<C / 64, true>;                            // the tail's layout
  static constexpr int TS = 16, PS = TS + 2, NPIX = PS * PS; // output tile side, patch side, patch pixels (324)
  static constexpr int PROWS = 384;                          // ... padded to 12 row blocks of 32
  static constexpr int CIN = 4 * C, NST1 = CIN / 32;         // conv1: K, its BK = 32 stages
  // patch image: [piece 2][k-group C / 8][row PROWS][8 f16]
  static constexpr int PKG = PROWS * 16, PPL = (C / 8) * PKG, PATCH = 2 * PPL;
  // phase 1 stages (H2Cfg's layouts; 32-B pad per k-group of A)
  static constexpr int AKG = PROWS * 16 + 32, APL = 4 * AKG, ASTG = 2 * APL;
  static constexpr int BKG = C * 16, BPL = 4 * BKG, STAGE_B = 2 * BPL;      // a weight stage (conv1 and conv2 alike): 8 KB
  static constexpr int W1OFF = 2 * ASTG, P1END = W1OFF + 2 * STAGE_B;
  static constexpr int RA = PROWS * 8 / 512;                 // A rows (16-byte loads) per thread and stage
  // phase 2: the weight ring behind the patch
  static constexpr int NRING = 4, RING = PATCH, P2END = RING + NRING * STAGE_B, NST2 = 9 * (C / 32);
  static constexpr int LDS0 = P1END > P2END ? P1END : P2END;
  static constexpr int RED = LDS0 > T::LDS ? LDS0 : T::LDS;  // the waves' patch maxima
  static constexpr int LDS = RED + 256;
  static_assert(LDS <= 160 * 1024 && STAGE_B == 8192 && PATCH <= W1OFF, "conv_block_kernel LDS");
};

// h2f_tail's rows for a 16 x 16 tile at (y0, x0) of image n: row r of the tile is pixel (y0 + r / 16, x0 + r % 16), so rows
// row0 + 64 s2 sit 4 image rows apart; a row is inside the image iff its column is and y0 + row0 / 16 + 4 s2 < H
struct BlockRows {
  int n, H, W, y0, x0;
  __device__ __forceinline__ H2fRows operator()(int row0) const {
    const int y = y0 + (row0 >> 4), x = x0 + (row0 & 15);
    return H2fRows{(unsigned)((n * H + y) * W + x), 4u * (unsigned)W, x < W ? (unsigned)y : 0x7fffff00u, 4u, (unsigned)H};
  }
};

template <int C, bool TRACE = false>
__global__ void __launch_bounds__(512, 2) conv_block_kernel(const ConvParams* __restrict__ pp, int first_round) {
  using G = BlockCfg<C>;
  using T = typename G::T;
  constexpr int PS = G::PS, NPIX = G::NPIX, PKG = G::PKG, PPL = G::PPL, AKG = G::AKG, APL = G::APL, ASTG = G::ASTG;
  constexpr int BKG = G::BKG, BPL = G::BPL, STAGE_B = G::STAGE_B, W1OFF = G::W1OFF, RA = G::RA, NST1 = G::NST1, NST2 = G::NST2;
  const ConvParams p = *pp;
  __shared__ __attribute__((aligned(16))) unsigned char lds[G::LDS];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fr = lane & 31, fg = lane >> 5;
  ODT_STAMP(0);
  // tiles in (image, tile row, tile column) order; an XCD takes a contiguous run of them (neighbours share their halo in its L2)
  int wg = (int)blockIdx.x;
  {
    const int nwg = (int)gridDim.x, xcd = wg & 7, q = nwg >> 3, r = nwg & 7;
    wg = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (wg >> 3);
  }
  // first-round stagger: a CU holds ONE workgroup, whose phases are memory-bound (1, 3) and matrix-bound (2) in turn.  The
  // workgroups of a launch start together and stay in step: every CU streams x at once (phase 1 ran at the chip's HBM rate, 16 us
  // per tile for 6 us of MFMAs), then every CU leaves HBM idle.  The first workgroup of a third of the CUs starts about one
  // third of a tile late (4 x s_sleep 127 = 15 us), that of another third two thirds: the thirds then meet HBM at different times
  // (b = 2 stamps: conv3 + stores 15.5 -> 11.1 us per tile; b = 8 @1080p: +0.7 FPS, inside the run-to-run spread:
  // profiles/block_fusion_res2_ab.txt).  ODT_FUSE_BLOCK=2: off (A/B).
  if ((p.debug & 0x200) == 0 && (int)blockIdx.x < first_round) {
    const int k = ((int)blockIdx.x >> 3) % 3;
    for (int i = 0; i < 4 * k; ++i) __builtin_amdgcn_s_sleep(127);
  }
  const int H = p.H, W = p.W;
  const int txn = (W + G::TS - 1) / G::TS, per_img = ((H + G::TS - 1) / G::TS) * txn;
  const int n_img = wg / per_img, t_img = wg - n_img * per_img, t_y = t_img / txn;
  const int y0 = t_y * G::TS, x0 = (t_img - t_y * txn) * G::TS;

  // =================================================================================================== phase 1: conv1
  const int sexp = h2_scale_exp(p.b_in_amax != nullptr ? amax_read(p.b_in_amax) : 0u);
  const float a_scale = pow2f(sexp), h2_inv = pow2f(-sexp);
  const __amdgpu_buffer_rsrc_t rs_in = __builtin_amdgcn_make_buffer_rsrc(
      (void*)p.b_in, 0, (int)((unsigned)p.B * H * W * (unsigned)p.b_in_ldc * 4u), 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_w1 = __builtin_amdgcn_make_buffer_rsrc((void*)p.b_wt, 0, NST1 * STAGE_B, 0x00020000);
  // K-slice rotation (conv_h2_kernel's, for the same reason): tile wg starts at slice wg mod 8 and wraps
  const int rot = (p.debug & 0x100) == 0 ? wg % NST1 : 0;
  auto dma_w1 = [&](int st, int boff) {
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_w1, ODT_LDS_PTR(lds + boff + wave * 1024), 16, lane * 16 + wave * 1024,
                                             (st + rot >= NST1 ? st + rot - NST1 : st + rot) * STAGE_B, 0, 0);
  };
  dma_w1(0, W1OFF);
  // loader: thread -> patch rows (t >> 3) + 64 j, 16-byte column t & 7 (eight lanes: the 128 bytes of a row's 32-channel slice);
  // patch row r = pixel (y0 - 1 + r / 18, x0 - 1 + r % 18); outside the image (or past the patch): out of range, zeros
  const int a_c = tid & 7, a_r = tid >> 3;
  int a_base[RA];
#pragma unroll
  for (int j = 0; j < RA; ++j) {
    const int pr = a_r + 64 * j, py = pr / PS, px = pr - py * PS;
    const int y = y0 - 1 + py, x = x0 - 1 + px;
    const bool ok = pr < NPIX && (unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W;
    a_base[j] = ok ? (int)((((unsigned)n_img * H + y) * W + x) * (unsigned)p.b_in_ldc * 4u + a_c * 16u) : (int)kOOB;
  }
  // (two stages of x in flight: stage st's rows sit in ga[st & 1] from the end of stage st - 3 to the end of stage st - 1)
  f32x4 ga[2][RA];
  auto load_a = [&](int st) {
    const int cs = st + rot >= NST1 ? st + rot - NST1 : st + rot;
#pragma unroll
    for (int j = 0; j < RA; ++j) ga[st & 1][j] = (f32x4)__builtin_amdgcn_raw_buffer_load_b128(rs_in, a_base[j], cs * 128, 0);
  };
  auto store_slot = [&](int st, int j) {
    const int abuf = (st & 1) * ASTG;
    const f32x4 g = ga[st & 1][j];
    unsigned h0, l0, h1, l1;
    split2h(g[0], g[1], a_scale, h0, l0);
    split2h(g[2], g[3], a_scale, h1, l1);
    unsigned char* d = lds + abuf + (a_c >> 1) * AKG + (a_r + 64 * j) * 16 + (a_c & 1) * 8;
    *reinterpret_cast<u32x2*>(d) = u32x2{h0, h1};
    *reinterpret_cast<u32x2*>(d + APL) = u32x2{l0, l1};
  };
  // conv1's epilogue constants of this lane's channels: register r of a tile = channel cb 32 + (r % 4) + 8 (r / 4) + 4 fg
  const int cb = wave & 1, rb0 = 3 * (wave >> 1);
  f32x4 sc1[4], bs1[4];
  {
    const __amdgpu_buffer_rsrc_t rs_ch = __builtin_amdgcn_make_buffer_rsrc((void*)p.b_chinv, 0, C * 4, 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_bs = __builtin_amdgcn_make_buffer_rsrc((void*)p.b_bias, 0, C * 4, 0x00020000);
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      sc1[g] = (f32x4)__builtin_amdgcn_raw_buffer_load_b128(rs_ch, (cb * 32 + 8 * g + 4 * fg) * 4, 0, 0) * h2_inv;
      bs1[g] = (f32x4)__builtin_amdgcn_raw_buffer_load_b128(rs_bs, (cb * 32 + 8 * g + 4 * fg) * 4, 0, 0);
    }
  }
  f32x16 acc1[3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc1[i][r] = 0.f;

  // prologue: stage 0 complete, stage 1's and 2's A in registers / in flight, stage 1's weights in flight behind the barrier
  load_a(0);
  load_a(1);
#pragma unroll
  for (int j = 0; j < RA; ++j) store_slot(0, j);
  ODT_WAIT_VM_LGKM0(RA);
  __builtin_amdgcn_s_barrier();
  dma_w1(1, W1OFF + STAGE_B);
  load_a(2);
  const int a_rd = fg * AKG + (rb0 * 32 + fr) * 16;
  const int w_rd = fg * BKG + (cb * 32 + fr) * 16;
  auto stage1 = [&](auto STC) {
    constexpr int st = decltype(STC)::value;
    constexpr int abuf = (st & 1) * ASTG, wbuf = W1OFF + (st & 1) * STAGE_B;
#pragma unroll
    for (int kst = 0; kst < 2; ++kst) {
      const f16x8 wh = *reinterpret_cast<const f16x8*>(lds + wbuf + kst * 2 * BKG + w_rd);
      const f16x8 wl = *reinterpret_cast<const f16x8*>(lds + wbuf + BPL + kst * 2 * BKG + w_rd);
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const f16x8 ah = *reinterpret_cast<const f16x8*>(lds + abuf + kst * 2 * AKG + a_rd + i * 512);
        const f16x8 al = *reinterpret_cast<const f16x8*>(lds + abuf + APL + kst * 2 * AKG + a_rd + i * 512);
        acc1[i] = ODT_MFMA_F16(wh, al, acc1[i]);             // lo * hi
        acc1[i] = ODT_MFMA_F16(wl, ah, acc1[i]);             // hi * lo
        acc1[i] = ODT_MFMA_F16(wh, ah, acc1[i]);             // hi * hi
      }
    }
    if constexpr (st + 1 < NST1) {
      // stage st + 1: registers -> LDS (its buffer was released by the previous barrier); its weights (requested a stage ago,
      // in front of stage st + 2's rows, which may stay in flight) have landed; behind the barrier the weights of stage st + 2
      // go into the buffer this stage leaves and the rows of stage st + 3 into the registers just stored
#pragma unroll
      for (int j = 0; j < RA; ++j) store_slot(st + 1, j);
      if constexpr (st + 2 < NST1) ODT_WAIT_VM_LGKM0(RA); else ODT_WAIT_VM_LGKM0(0);
      __builtin_amdgcn_s_barrier();
      if constexpr (st + 2 < NST1) dma_w1(st + 2, wbuf);
      if constexpr (st + 3 < NST1) load_a(st + 3);
    }
  };
  stage1(std::integral_constant<int, 0>{}); stage1(std::integral_constant<int, 1>{}); stage1(std::integral_constant<int, 2>{});
  stage1(std::integral_constant<int, 3>{}); stage1(std::integral_constant<int, 4>{}); stage1(std::integral_constant<int, 5>{});
  stage1(std::integral_constant<int, 6>{}); stage1(std::integral_constant<int, 7>{});
  static_assert(NST1 == 8, "conv1 stages");
  ODT_STAMP(1);

  // ---- conv1's epilogue in registers; the tile's power of two; the patch image
  float mx = 0.f;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const int pr = (rb0 + i) * 32 + fr, py = pr / PS, px = pr - py * PS;
    const bool ok = pr < NPIX && (unsigned)(y0 - 1 + py) < (unsigned)H && (unsigned)(x0 - 1 + px) < (unsigned)W;
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float v = acc1[i][4 * g + e] * sc1[g][e];
        v += bs1[g][e];
        v = ok ? fmaxf(v, 0.f) : 0.f;
        acc1[i][4 * g + e] = v;
        mx = fmaxf(mx, v);
      }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) mx = fmaxf(mx, __shfl_xor(mx, d));
  float* red = reinterpret_cast<float*>(lds + G::RED);
  if (lane == 0) red[wave] = mx;
  ODT_BARRIER_LDS();                        // (also: every wave has left the last stage -- the A / W buffers are dead)
  // conv2's weight stream: stage = (32-channel slice, tap), NRING - 1 stages ahead
  const __amdgpu_buffer_rsrc_t rs_w2 = __builtin_amdgcn_make_buffer_rsrc((void*)p.b_wt2, 0, NST2 * STAGE_B, 0x00020000);
  auto dma_w2 = [&](int st) {
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_w2, ODT_LDS_PTR(lds + G::RING + (st & (G::NRING - 1)) * STAGE_B + wave * 1024), 16,
                                             lane * 16 + wave * 1024, st * STAGE_B, 0, 0);
  };
  dma_w2(0); dma_w2(1); dma_w2(2);
  float t_inv;                              // 2^-e of the tile
  {
    const f32x4 r0 = *reinterpret_cast<const f32x4*>(red), r1 = *reinterpret_cast<const f32x4*>(red + 4);
    const float m = fmaxf(fmaxf(fmaxf(r0[0], r0[1]), fmaxf(r0[2], r0[3])), fmaxf(fmaxf(r1[0], r1[1]), fmaxf(r1[2], r1[3])));
    const int be = (int)((__float_as_uint(m) >> 23) & 0xffu);
    int e = 14 - (be - 127);
    e = e > 100 ? 100 : (e < -100 ? -100 : e);
    e = ((be == 0) | (be == 255)) ? 0 : e;
    const float t_scale = pow2f(e);
    t_inv = pow2f(-e);
    // registers 8 h .. 8 h + 7 of a tile are k-group cb 4 + 2 h + fg of the lane's patch row
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      unsigned char* d = lds + (cb * 4 + fg) * PKG + ((rb0 + i) * 32 + fr) * 16;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        u32x4 hq, lq;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          unsigned a, b;
          split2h(acc1[i][8 * h + 2 * t], acc1[i][8 * h + 2 * t + 1], t_scale, a, b);
          hq[t] = a; lq[t] = b;
        }
        *reinterpret_cast<u32x4*>(d + 2 * h * PKG) = hq;
        *reinterpret_cast<u32x4*>(d + 2 * h * PKG + PPL) = lq;
      }
    }
  }
  // the constants the tail reads from LDS: this conv's 2^-e 2^-t_c and bias, conv3's 2^-t_n and bias (stored behind phase 2:
  // their places lie inside the patch)
  f32x4 kcv, k3v;
  {
    const int q = tid & 63;
    const __amdgpu_buffer_rsrc_t rs_ch = __builtin_amdgcn_make_buffer_rsrc((void*)p.h2_chinv, 0, C * 4, 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_bias = __builtin_amdgcn_make_buffer_rsrc((void*)p.bias, 0, C * 4, 0x00020000);
    kcv = tid < 64 ? (f32x4)__builtin_amdgcn_raw_buffer_load_b128(rs_ch, q * 16, 0, 0) * t_inv
                   : (f32x4)__builtin_amdgcn_raw_buffer_load_b128(rs_bias, tid < 128 ? q * 16 : (int)kOOB, 0, 0);
    const __amdgpu_buffer_rsrc_t rs_k3 = __builtin_amdgcn_make_buffer_rsrc((void*)(tid < 256 ? p.f_chinv : p.f_bias), 0, (int)((unsigned)p.f_cout * 4u), 0x00020000);
    k3v = (f32x4)__builtin_amdgcn_raw_buffer_load_b128(rs_k3, (tid & 255) * 16, 0, 0);
  }
  ODT_BARRIER_LDS();                        // the patch is complete
  ODT_STAMP(2);

  // =================================================================================================== phase 2: conv2
  const int wm = wave >> 1, wn = wave & 1;
  f32x16 acc[2][1];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[i][0][r] = 0.f;
  // lane's pixels: tile rows wm 64 + i 32 + fr = tile pixel (wm 4 + i 2 + fr / 16, fr % 16); tap (kh, kw) of it is patch row + kh 18 + kw
  const int p_rd = fg * PKG + ((wm * 4 + (fr >> 4)) * PS + (fr & 15)) * 16;
  const int b_rd = fg * BKG + (wn * 32 + fr) * 16;
  auto stage2 = [&](auto STC) {
    constexpr int st = decltype(STC)::value;
    constexpr int cs = st / 9, tap = st % 9, kh = tap / 3, kw = tap % 3;
    // stage st's weights have landed (younger DMAs may fly); the barrier also releases the slot stage st - 1 was read from
    if constexpr (st + 2 < NST2) ODT_WAIT_VM_LGKM0(2); else if constexpr (st + 1 < NST2) ODT_WAIT_VM_LGKM0(1); else ODT_WAIT_VM_LGKM0(0);
    __builtin_amdgcn_s_barrier();
    if constexpr (st + 3 < NST2) dma_w2(st + 3);
    const unsigned char* wb = lds + G::RING + (st & (G::NRING - 1)) * STAGE_B + b_rd;
    const unsigned char* pa = lds + cs * 4 * PKG + (kh * PS + kw) * 16 + p_rd;
#pragma unroll
    for (int kst = 0; kst < 2; ++kst) {
      const f16x8 wh = *reinterpret_cast<const f16x8*>(wb + kst * 2 * BKG);
      const f16x8 wl = *reinterpret_cast<const f16x8*>(wb + BPL + kst * 2 * BKG);
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const f16x8 ah = *reinterpret_cast<const f16x8*>(pa + kst * 2 * PKG + i * 2 * PS * 16);
        const f16x8 al = *reinterpret_cast<const f16x8*>(pa + PPL + kst * 2 * PKG + i * 2 * PS * 16);
        acc[i][0] = ODT_MFMA_F16(wh, al, acc[i][0]);         // lo * hi
        acc[i][0] = ODT_MFMA_F16(wl, ah, acc[i][0]);         // hi * lo
        acc[i][0] = ODT_MFMA_F16(wh, ah, acc[i][0]);         // hi * hi
      }
    }
  };
  stage2(std::integral_constant<int, 0>{}); stage2(std::integral_constant<int, 1>{}); stage2(std::integral_constant<int, 2>{});
  stage2(std::integral_constant<int, 3>{}); stage2(std::integral_constant<int, 4>{}); stage2(std::integral_constant<int, 5>{});
  stage2(std::integral_constant<int, 6>{}); stage2(std::integral_constant<int, 7>{}); stage2(std::integral_constant<int, 8>{});
  stage2(std::integral_constant<int, 9>{}); stage2(std::integral_constant<int, 10>{}); stage2(std::integral_constant<int, 11>{});
  stage2(std::integral_constant<int, 12>{}); stage2(std::integral_constant<int, 13>{}); stage2(std::integral_constant<int, 14>{});
  stage2(std::integral_constant<int, 15>{}); stage2(std::integral_constant<int, 16>{}); stage2(std::integral_constant<int, 17>{});
  static_assert(NST2 == 18, "conv2 stages");
  ODT_BARRIER_LDS();                        // every wave has left the patch and the ring
  if (tid < 128) *reinterpret_cast<f32x4*>(lds + T::F_KOFF + (tid >> 6) * 1024 + (tid & 63) * 16) = kcv;
  *reinterpret_cast<f32x4*>(lds + T::F_K3OFF + (tid >> 8) * 4096 + (tid & 255) * 16) = k3v;
  ODT_BARRIER_LDS();
  ODT_STAMP(6);

  // =================================================================================================== phase 3: conv3
  h2f_tail<1, TRACE>(p, acc, lds, wg * 256, p.B * H * W, wave, wm, wn, 0.f, BlockRows{n_img, H, W, y0, x0});
  ODT_STAMP(5);
}

}  // namespace

// c1: the 1x1 conv 4C -> C (ReLU) on a 64-wide fp16x2 n-tile; c2: the dense 3x3 conv C -> C reading it, already carrying the
// fused tail (conv_h2f_fusable) whose same-shape shortcut is c1's input
bool conv_block_fits(const ConvParams& c1, const ConvParams& c2) {
  const ConvKernelRow& r1 = conv_variant_row(c1.variant);
  const ConvKernelRow& r2 = conv_variant_row(c2.variant);
  const bool c1_ok = c1.wt_split != nullptr && r1.family == CF_H2 && r1.bn == 64 && r1.flags == 0 && c1.h2_chinv != nullptr && c1.kh == 1 && c1.kw == 1 &&
                     c1.stride == 1 && c1.pad_t == 0 && c1.pad_l == 0 && c1.Cout == 64 && c1.Cin == 256 && c1.relu == 1 && c1.in2 == nullptr &&
                     c1.splitk <= 1 && c1.res_mode == 0 && c1.nlvl <= 1 && c1.head_wt == nullptr && c1.f_wt == nullptr && c1.in_amax != nullptr &&
                     c1.H == c1.in_Ha && c1.W == c1.in_Wa && c1.Ho == c1.H && c1.Wo == c1.W && c1.out_oy == 0 && c1.out_ox == 0 &&
                     c1.out_H == c1.Ho && c1.out_W == c1.Wo && c1.in_ldc % 4 == 0 && c1.in_ldc >= c1.Cin;
  const bool c2_ok = c2.wt_split != nullptr && r2.family == CF_H2 && r2.bn == 64 && (r2.flags & CVF_FTAIL) != 0 && c2.f_wt != nullptr && c2.in == c1.out &&
                     c2.kh == 3 && c2.kw == 3 && c2.stride == 1 && c2.dil == 1 && c2.pad_t == 1 && c2.pad_l == 1 && c2.Cin == 64 && c2.Cout == 64 &&
                     c2.relu == 1 && c2.B == c1.B && c2.H == c1.Ho && c2.W == c1.Wo && c2.Ho == c2.H && c2.Wo == c2.W && c2.f_cout == 256 &&
                     c2.f_res == c1.in && c2.f_res_ldc == c1.in_ldc && c2.f_out != nullptr &&
                     (double)c2.B * c2.H * c2.W * (double)(c1.in_ldc > c2.f_out_ldc ? c1.in_ldc : c2.f_out_ldc) * 4.0 < 2147483648.0;
  return c1_ok && c2_ok;
}

void conv_block_fuse(ConvParams& c2, const ConvParams& c1, const void* img_p) {
  c2.b_in = c1.in; c2.b_in_ldc = c1.in_ldc; c2.b_cin = c1.Cin; c2.b_wt = c1.wt_split; c2.b_chinv = c1.h2_chinv;
  c2.b_bias = c1.bias; c2.b_in_amax = c1.in_amax; c2.b_wt2 = img_p;
  c2.in = c1.in; c2.in_amax = c1.in_amax;        // (conv1's output does not exist: the record names real memory only)
  c2.debug |= c1.debug & 0x100;
}

int launch_bottleneck_block(const ConvParams& p, const ConvParams* dev, hipStream_t stream) {
  ODT_CHECK(p.b_in != nullptr && p.b_wt != nullptr && p.b_wt2 != nullptr && p.b_chinv != nullptr && p.b_bias != nullptr && p.f_wt != nullptr &&
                p.f_out != nullptr && p.h2_chinv != nullptr && p.Cin == 64 && p.Cout == 64 && p.b_cin == 256 && p.f_cout == 256 && p.kh == 3 && p.kw == 3 &&
                p.dil == 1 && p.stride == 1 && p.Ho == p.H && p.Wo == p.W,
            "bottleneck block: the record is not a 64-wide identity bottleneck");
  ODT_CHECK((double)p.B * p.H * p.W * (double)(p.b_in_ldc > p.f_out_ldc ? p.b_in_ldc : p.f_out_ldc) * 4.0 < 2147483648.0,
            "bottleneck block: tensor of 2 GiB or more");
  const unsigned grid = (unsigned)p.B * (unsigned)((p.H + 15) / 16) * (unsigned)((p.W + 15) / 16);
  // workgroups of the first round: one per CU of the current device (conv_stem_grid's per-device table)
  static std::atomic<int> cus[64];
  int dev_id = 0;
  ODT_HIP(hipGetDevice(&dev_id));
  int ncu = dev_id >= 0 && dev_id < 64 ? cus[dev_id].load(std::memory_order_relaxed) : 0;
  if (ncu == 0) {
    hipDeviceProp_t prop;
    ODT_HIP(hipGetDeviceProperties(&prop, dev_id));
    ncu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    if (dev_id >= 0 && dev_id < 64) cus[dev_id].store(ncu, std::memory_order_relaxed);
  }
  // (p.trace: per-workgroup phase stamps [0] start, [1] conv1's loop done, [2] patch complete, [6] conv2 done, [3] the tail's pieces
  // ready, [5] end -- ODT_CONV_TRACE, tuning only)
  if (p.trace != nullptr) hipLaunchKernelGGL((conv_block_kernel<64, true>), dim3(grid), dim3(512), 0, stream, dev, ncu);
  else hipLaunchKernelGGL((conv_block_kernel<64, false>), dim3(grid), dim3(512), 0, stream, dev, ncu);
  ODT_HIP(hipGetLastError());
  return 0;
}

}  // namespace odt
