// 3x3 grouped convolution, 32 groups, NHWC f32 (ResNeXt-32x4d: conv2 of resnext_32x4d_bottleneck, reference nn.py:524-549):
//   out[b, yo, xo, o] = act(bias[o] + sum_{ky, kx, i < G} in[b, yo s + ky d - pad_t, xo s + kx d - pad_l, (o / G) G + i] w[ky][kx][i][o])
// with C = Cin = Cout in {128, 256, 512, 1024}, G = C / 32 in {4, 8, 16, 32}, stride s and dilation d in {1, 2}; taps outside
// H x W contribute zero (TensorFlow's 'SAME' pads after as well as before).  Plain f32 in every arithmetic mode -- the layer is
// 1 / 32 of a dense 3x3's work and bound by its tensors, not by its products -- summed in one fixed order (kernel rows outermost),
// so that two runs are bit-identical.  The |max| of what is stored goes to the output's range slot, as from a conv epilogue.
//   G = 4, 8    group_conv_stream_kernel: dwconv_kernel's scheme (effnet.hip).  A thread owns one output channel quad and PX
//               horizontally adjacent outputs; 16-byte accesses, channels innermost; the input columns of a kernel row are
//               loaded once and reused by the PX outputs.  Weights as HWIO [3][3][G][C]: the quad's four weights of
//               (tap, i) are one 16-byte load.
//   G = 16, 32  group_conv_mfma_kernel: per group a GEMM with K = 9 G, N = G on v_mfma_f32_16x16x4_f32 (a k-ordered fmaf chain:
//               exact f32).  A wave owns 16 output channels and keeps their 9 G x 16 weights in registers; the MFMA's A
//               operand is the weights, B the pixels, so that a lane ends with four adjacent channels of one pixel: one
//               16-byte store.  Two 16-pixel tiles per step: two independent accumulators cover the MFMA's latency.
// Built with -ffp-contract=off.
#include "conv_split_epilogue.hpp"

namespace odt {
namespace {

constexpr int group_px(int S) { return S == 1 ? 4 : 2; }

template <int G, int S, int D>
__global__ void __launch_bounds__(256, 4) group_conv_stream_kernel(GroupConvParams p) {
  constexpr int PX = group_px(S), NC = (PX - 1) * S + 2 * D + 1, GQ = G / 4;
  __shared__ float red[4];
  const int tid = threadIdx.x;
  const int c4n = p.C >> 2, nxb = (p.Wo + PX - 1) / PX;
  const long total = (long)p.B * p.Ho * nxb * c4n;
  const long idx = (long)blockIdx.x * 256 + tid;
  float vmax = 0.f;
  if (idx < total) {
    const int c4 = (int)(idx % c4n);
    long u = idx / c4n;
    const int xb = (int)(u % nxb); u /= nxb;
    const int yo = (int)(u % p.Ho), b = (int)(u / p.Ho);
    const int ci0 = (c4 * 4 / G) * G;                 // first input channel of the quad's group
    const int xo0 = xb * PX, x0 = xo0 * S - p.pad_l;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    f32x4 acc[PX];
#pragma unroll
    for (int q = 0; q < PX; ++q) acc[q] = zero;
    // (rolled: unrolled, the compiler hoists every tap's weight loads to the top and the kernel loses its waves to registers)
#pragma unroll 1
    for (int ky = 0; ky < 3; ++ky) {
      const int y = yo * S + ky * D - p.pad_t;
      if ((unsigned)y >= (unsigned)p.H) continue;
      const int row = ((b * p.H + y) * p.W) * p.C + ci0;      // (32-bit element offsets from the uniform base: launch_group_conv checks)
      // one quad of the group's input channels at a time: its NC columns live in registers only as long as the quad's taps run
#pragma unroll 1
      for (int h = 0; h < GQ; ++h) {
        f32x4 col[NC];
#pragma unroll
        for (int cidx = 0; cidx < NC; ++cidx) {
          const int x = x0 + cidx;
          col[cidx] = (unsigned)x < (unsigned)p.W ? *reinterpret_cast<const f32x4*>(p.in + (row + x * p.C + h * 4)) : zero;
        }
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
          const int wo = ((ky * 3 + kx) * G + h * 4) * p.C + c4 * 4;
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const f32x4 w = *reinterpret_cast<const f32x4*>(p.wt + (wo + i * p.C));
#pragma unroll
            for (int q = 0; q < PX; ++q) acc[q] = acc[q] + col[q * S + kx * D][i] * w;
          }
        }
      }
    }
    const f32x4 bias = *reinterpret_cast<const f32x4*>(p.bias + c4 * 4);
    const int orow = ((b * p.Ho + yo) * p.Wo) * p.C + c4 * 4;
#pragma unroll
    for (int q = 0; q < PX; ++q) {
      const int xo = xo0 + q;
      if (xo >= p.Wo) break;
      f32x4 v = acc[q] + bias;
      if (p.relu) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
      }
      *reinterpret_cast<f32x4*>(p.out + (orow + xo * p.C)) = v;
      vmax = fmaxf(vmax, fmaxf(fmaxf(fabsf(v[0]), fabsf(v[1])), fmaxf(fabsf(v[2]), fabsf(v[3]))));
    }
  }
  publish_amax_wg<256>(p.out_amax, vmax, tid, reinterpret_cast<unsigned char*>(red));
}

// grid (pixel-tile walkers, C / 64): wave w of workgroup (., cy) owns output channels [16 nt, 16 nt + 16), nt = 4 cy + w, and
// walks the 32-pixel tiles (b, yo, 32 xt ...) with the stride of the grid's x extent.  Lane l: pixel l & 15 of either half
// tile, k slot l >> 4.  One 16-byte load of a tap gives input channels 4 (l >> 4) + e (+ 16 h), e = 0..3: MFMA e of the tap
// sums over them, and the weight image (group_conv_pack_weights) holds the matching w[tap][16 h + 4 (l >> 4) + e][16 nt + (l & 15)]
// as element e of lane l's 16 bytes.
template <int G>
__global__ void __launch_bounds__(256) group_conv_mfma_kernel(GroupConvParams p) {
  constexpr int KH = G / 16;
  __shared__ float red[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nt = (int)blockIdx.y * 4 + wave;
  const int px = lane & 15, kq = lane >> 4;
  const int ci = (nt * 16 / G) * G + kq * 4;          // + 16 h
  f32x4 w[9][KH];
  {
    const f32x4* img = reinterpret_cast<const f32x4*>(p.wt) + (long)nt * 9 * KH * 64 + lane;
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
      for (int h = 0; h < KH; ++h) w[t][h] = img[(t * KH + h) * 64];
  }
  const f32x4 bias = *reinterpret_cast<const f32x4*>(p.bias + nt * 16 + kq * 4);
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  const int nxt = (p.Wo + 31) >> 5;
  const long tiles = (long)p.B * p.Ho * nxt;
  float vmax = 0.f;
  for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int xt = (int)(tile % nxt);
    const long u = tile / nxt;
    const int yo = (int)(u % p.Ho), b = (int)(u / p.Ho);
    const int xo = xt * 32 + px;                      // and xo + 16
    f32x4 acc0 = zero, acc1 = zero;
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
      const int y = yo * p.stride + ky * p.dil - p.pad_t;
      const bool yin = (unsigned)y < (unsigned)p.H;
      const float* row = p.in + (((long)b * p.H + (yin ? y : 0)) * p.W) * p.C + ci;
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        const int xa = xo * p.stride + kx * p.dil - p.pad_l, xb = xa + 16 * p.stride;
        const bool ina = yin && xo < p.Wo && (unsigned)xa < (unsigned)p.W;
        const bool inb = yin && xo + 16 < p.Wo && (unsigned)xb < (unsigned)p.W;
#pragma unroll
        for (int h = 0; h < KH; ++h) {
          const f32x4 va = ina ? *reinterpret_cast<const f32x4*>(row + (long)xa * p.C + h * 16) : zero;
          const f32x4 vb = inb ? *reinterpret_cast<const f32x4*>(row + (long)xb * p.C + h * 16) : zero;
          const f32x4 wv = w[ky * 3 + kx][h];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[e], va[e], acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[e], vb[e], acc1, 0, 0, 0);
          }
        }
      }
    }
    // D register r of lane l: row (output channel) 4 (l >> 4) + r, column (pixel) l & 15
    float* orow = p.out + (((long)b * p.Ho + yo) * p.Wo) * p.C + nt * 16 + kq * 4;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      const int x = xo + 16 * half;
      if (x >= p.Wo) continue;
      f32x4 v = (half == 0 ? acc0 : acc1) + bias;
      if (p.relu) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
      }
      *reinterpret_cast<f32x4*>(orow + (long)x * p.C) = v;
      vmax = fmaxf(vmax, fmaxf(fmaxf(fabsf(v[0]), fabsf(v[1])), fmaxf(fabsf(v[2]), fabsf(v[3]))));
    }
  }
  publish_amax_wg<256>(p.out_amax, vmax, tid, reinterpret_cast<unsigned char*>(red));
}

template <int G>
void launch_stream(const GroupConvParams& p, hipStream_t stream) {
  auto go = [&](auto kern, int px) {
    const long total = (long)p.B * p.Ho * ((p.Wo + px - 1) / px) * (p.C / 4);
    hipLaunchKernelGGL(kern, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, p);
  };
  if (p.stride == 1 && p.dil == 1) go(group_conv_stream_kernel<G, 1, 1>, group_px(1));
  else if (p.stride == 1) go(group_conv_stream_kernel<G, 1, 2>, group_px(1));
  else if (p.dil == 1) go(group_conv_stream_kernel<G, 2, 1>, group_px(2));
  else go(group_conv_stream_kernel<G, 2, 2>, group_px(2));
}

template <int G>
void launch_mfma(const GroupConvParams& p, hipStream_t stream) {
  // every wave loads its 9 G x 16 weights once: enough tiles per walker to pay for them, enough walkers to fill the chip
  const long tiles = (long)p.B * p.Ho * ((p.Wo + 31) / 32);
  const long gx = std::min<long>(tiles, std::max<long>(1, 4096 / (p.C / 64)));
  hipLaunchKernelGGL(group_conv_mfma_kernel<G>, dim3((unsigned)gx, p.C / 64), dim3(256), 0, stream, p);
}

}  // namespace

size_t group_conv_weight_elems(int C) { return (size_t)9 * (C / 32) * C; }

// HWIO [3][3][G][C] (* scale[o]: the folded BN, in double, rounded once) -> the kernels' image, group_conv_weight_elems(C)
// floats.  G = 4, 8: the same order.  G = 16, 32: [C / 16][9][G / 16][64 lanes][4] (group_conv_mfma_kernel).
int group_conv_pack_weights(const float* hwio, const double* scale, int C, float* dst) {
  ODT_CHECK(C == 128 || C == 256 || C == 512 || C == 1024, "group conv: C must be 128, 256, 512 or 1024");
  const int G = C / 32;
  auto src = [&](int t, int i, int o) { return (float)((double)hwio[((size_t)t * G + i) * C + o] * (scale ? scale[o] : 1.0)); };
  if (G < 16) {
    for (int t = 0; t < 9; ++t)
      for (int i = 0; i < G; ++i)
        for (int o = 0; o < C; ++o) dst[((size_t)t * G + i) * C + o] = src(t, i, o);
    return 0;
  }
  const int KH = G / 16;
  for (int nt = 0; nt < C / 16; ++nt)
    for (int t = 0; t < 9; ++t)
      for (int h = 0; h < KH; ++h)
        for (int l = 0; l < 64; ++l)
          for (int e = 0; e < 4; ++e)
            dst[((((size_t)nt * 9 + t) * KH + h) * 64 + l) * 4 + e] = src(t, 16 * h + 4 * (l >> 4) + e, 16 * nt + (l & 15));
  return 0;
}

int launch_group_conv(const GroupConvParams& p, hipStream_t stream) {
  ODT_CHECK(p.in && p.wt && p.bias && p.out, "group conv: null argument");
  ODT_CHECK(p.C == 128 || p.C == 256 || p.C == 512 || p.C == 1024, "group conv: C must be 128, 256, 512 or 1024");
  ODT_CHECK(p.B >= 1 && p.H >= 1 && p.W >= 1 && p.Ho >= 1 && p.Wo >= 1 && (p.stride == 1 || p.stride == 2) &&
            (p.dil == 1 || p.dil == 2) && p.pad_t >= 0 && p.pad_l >= 0, "group conv: bad geometry");
  // the last output's first tap lies inside the padded input (nothing indexes past what the bounds checks cover anyway)
  ODT_CHECK((long)(p.Ho - 1) * p.stride - p.pad_t < p.H && (long)(p.Wo - 1) * p.stride - p.pad_l < p.W,
            "group conv: output larger than the input allows");
  // (the streaming kernel addresses both tensors with 32-bit element offsets)
  ODT_CHECK((double)p.B * p.H * p.W * p.C < 2147483648.0 && (double)p.B * p.Ho * p.Wo * p.C < 2147483648.0,
            "group conv: a tensor reaches 2^31 elements");
  switch (p.C / 32) {
    case 4: launch_stream<4>(p, stream); break;
    case 8: launch_stream<8>(p, stream); break;
    case 16: launch_mfma<16>(p, stream); break;
    default: launch_mfma<32>(p, stream); break;
  }
  ODT_HIP(hipGetLastError());
  return 0;
}

}  // namespace odt
