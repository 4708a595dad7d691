// Deformable 3x3 convolution of a stage-entry bottleneck (--use_deformable; reference nn.py:469-485, :1642-1712 and
// deformable_helper.py), NHWC f32.  Two kernels, launched one after the other by launch_deform_conv:
//   deform_offset_kernel   conv2_offset: the 18 offset channels at the EVEN input positions only (the deformable conv reads no
//                          others): a 3x3 stride-2 conv with one zero row / column in front, C -> 18, + bias.
//                          off[b, yo, xo, 2 n] is the row offset of tap n = 3 ky + kx, off[.., 2 n + 1] its column offset.
//   deform_conv_kernel     out[b, yo, xo, :] = sum_n sum_ci s[n, ci] W[ky, kx, ci, :] with s the bilinear sample of the input at
//                            r = clip(f32(2 yo - 1 + ky) + off[2 n], 0, H - 1)      c = clip(f32(2 xo - 1 + kx) + off[2 n + 1], 0, W - 1)
//                            vt = x[r0,c0] + (x[r1,c0] - x[r0,c0]) fr      vb = x[r0,c1] + (x[r1,c1] - x[r0,c1]) fr      s = vt + (vb - vt) fc
//                          (r0 / r1 = floor / ceil of r, fr = r - r0; the border is a clamp of the coordinate, not zero padding; no
//                          bias, no BN, no activation: the output is signed).  Each image uses its own offsets.
// Both are GEMMs on v_mfma_f32_32x32x2_f32 (a k-ordered fmaf chain: exact f32) in every arithmetic mode, summed in one fixed
// order, so that two runs are bit-identical.  The MFMA's A operand is the weights and B the pixels: a lane ends with four
// adjacent channels of one pixel, one 16-byte store.
//
// deform_conv_kernel: a workgroup owns 32 consecutive output pixels (of the flattened [B Ho Wo]) across ALL C output channels,
// so that every sample is gathered once; wave w owns output channels [w C / 4, (w + 1) C / 4) -- C / 128 accumulator tiles of
// 32 x 32, 64 registers at C = 512.  The nine coordinate pairs of each pixel are computed once, into LDS (four corner element
// offsets + the two fractions).  K runs over (tap, 64-channel slice): the 256 threads gather the four corner runs of the slice
// with 16-byte loads (a corner is a contiguous run of C floats), interpolate in the order above and stage the 32 x 64 sampled
// operand in LDS, twice buffered: the gathers of slice k + 1 are in flight under the MFMAs of slice k, one barrier per slice.
// The LDS image is [channel quad q][pixel ^ q][4]: the MFMA lane (pixel i, k half h) reads quad 2 m + h as one ds_read_b128,
// the XOR keeps the staging writes of 16 lanes that share a pixel off each other's banks.  The weights come straight from
// global memory / L2 as 16-byte loads of a packed image (deform_pack_weights): no wave shares another's.
// Built with -ffp-contract=off.
#include "conv_split_epilogue.hpp"

namespace odt {
namespace {

constexpr int kDfPx = 32;      // output pixels per workgroup
constexpr int kDfKC = 64;      // channels per staged slice
constexpr int kDfQ = kDfKC / 4;

// grid: ceil(M / 32).  Wave w sums channels [w C / 4, (w + 1) C / 4) of every tap; the four partial tiles meet in LDS and are
// added in wave order, then the bias.  Lane l: pixel l & 31, k half l >> 5; D register r: output channel (r & 3) + 8 (r >> 2) +
// 4 (l >> 5) of 32 (18 used; the image's other rows are zero).
__global__ void __launch_bounds__(256) deform_offset_kernel(DeformConvParams p) {
  __shared__ float red[4 * 16 * 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int px = lane & 31, h = lane >> 5;
  const int HoWo = p.Ho * p.Wo, M = p.B * HoWo;
  const int pix = (int)blockIdx.x * kDfPx + px;
  const bool valid = pix < M;
  int b = 0, yo = 0, xo = 0;
  if (valid) { b = pix / HoWo; const int r = pix - b * HoWo; yo = r / p.Wo; xo = r - yo * p.Wo; }
  const int mw = p.C >> 5;                             // 8-channel steps per wave
  const int m0 = wave * mw;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  const f32x4* img = reinterpret_cast<const f32x4*>(p.wt_off) + lane;
  for (int ky = 0; ky < 3; ++ky) {
    const int y = 2 * yo - 1 + ky;
    const bool yin = valid && (unsigned)y < (unsigned)p.H;
    for (int kx = 0; kx < 3; ++kx) {
      const int x = 2 * xo - 1 + kx;
      const bool in = yin && (unsigned)x < (unsigned)p.W;
      // (32-bit element offsets: launch_deform_conv checks)
      const float* src = p.in + (((b * p.Ha + (in ? y : 0)) * p.Wa + (in ? x : 0)) * p.ldc + 4 * h);
      const f32x4* wimg = img + (size_t)((ky * 3 + kx) * (p.C >> 3) + m0) * 64;
      for (int m = 0; m < mw; ++m) {
        const f32x4 v = in ? *reinterpret_cast<const f32x4*>(src + 8 * (m0 + m)) : zero;
        const f32x4 wv = wimg[m * 64];
#pragma unroll
        for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wv[e], v[e], acc, 0, 0, 0);
      }
    }
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) red[(wave * 16 + r) * 64 + lane] = acc[r];
  __syncthreads();
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int idx = tid + 256 * u, r = idx >> 6, l = idx & 63;
    const int j = (r & 3) + 8 * (r >> 2) + 4 * (l >> 5);
    const int q = (int)blockIdx.x * kDfPx + (l & 31);
    if (j < 18 && q < M) {
      const float s = ((red[r * 64 + l] + red[(16 + r) * 64 + l]) + red[(32 + r) * 64 + l]) + red[(48 + r) * 64 + l];
      p.off[q * 18 + j] = s + p.b_off[j];
    }
  }
}

template <int NT>
__global__ void __launch_bounds__(256, 2) deform_conv_kernel(DeformConvParams p) {
  constexpr int C = 128 * NT, NSL = C / kDfKC, NCHUNK = 9 * NSL;
  constexpr int SMP = kDfQ * kDfPx * 4;                // floats per staging buffer
  __shared__ __attribute__((aligned(16))) float lds[2 * SMP + 6 * 9 * kDfPx];
  int* cof = reinterpret_cast<int*>(lds + 2 * SMP);    // [tap][pixel][4]: element offsets of (r0,c0) (r1,c0) (r0,c1) (r1,c1)
  float* cfr = lds + 2 * SMP + 4 * 9 * kDfPx;          // [tap][pixel][2]: fr, fc
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int HoWo = p.Ho * p.Wo, M = p.B * HoWo;
  const int pix0 = (int)blockIdx.x * kDfPx;

  // ---- the nine coordinate pairs of each pixel, once
  for (int it = tid; it < 9 * kDfPx; it += 256) {
    const int i = it & (kDfPx - 1), n = it >> 5;
    const int pix = pix0 + i;
    int o[4] = {0, 0, 0, 0};
    float fr = 0.f, fc = 0.f;
    if (pix < M) {       // (a pixel past the end samples element 0 and is not stored)
      const int b = pix / HoWo, rem = pix - b * HoWo, yo = rem / p.Wo, xo = rem - yo * p.Wo;
      const int ky = n / 3, kx = n - 3 * ky;
      const float* of = p.off + (pix * 18 + 2 * n);
      // one f32 addition, then the clamp (NaN clamps to 0: fmaxf drops it)
      const float r = fminf(fmaxf((float)(2 * yo - 1 + ky) + of[0], 0.f), (float)(p.H - 1));
      const float c = fminf(fmaxf((float)(2 * xo - 1 + kx) + of[1], 0.f), (float)(p.W - 1));
      const float r0f = floorf(r), c0f = floorf(c);
      const int r0 = (int)r0f, r1 = (int)ceilf(r), c0 = (int)c0f, c1 = (int)ceilf(c);
      fr = r - r0f; fc = c - c0f;
      const int row0 = (b * p.Ha + r0) * p.Wa, row1 = (b * p.Ha + r1) * p.Wa;
      o[0] = (row0 + c0) * p.ldc; o[1] = (row1 + c0) * p.ldc; o[2] = (row0 + c1) * p.ldc; o[3] = (row1 + c1) * p.ldc;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) cof[it * 4 + k] = o[k];
    cfr[it * 2] = fr; cfr[it * 2 + 1] = fc;
  }
  __syncthreads();

  // staging: item = tid + 256 u -> channel quad q = item & 15 of the slice, pixel i = item >> 4
  const int sq = tid & (kDfQ - 1), si = tid >> 4;      // (+ 16 pixels for u = 1)
  f32x4 g[2][4];
  auto gather = [&](int chunk) {
    const int n = chunk / NSL, sl = chunk - n * NSL;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int* o = cof + (n * kDfPx + si + 16 * u) * 4;
      const float* src = p.in + (sl * kDfKC + 4 * sq);
#pragma unroll
      for (int k = 0; k < 4; ++k) g[u][k] = *reinterpret_cast<const f32x4*>(src + o[k]);
    }
  };
  auto stage = [&](int chunk, float* buf) {
    const int n = chunk / NSL;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int i = si + 16 * u;
      const float fr = cfr[(n * kDfPx + i) * 2], fc = cfr[(n * kDfPx + i) * 2 + 1];
      f32x4 s;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float vt = g[u][0][e] + (g[u][1][e] - g[u][0][e]) * fr;
        const float vb = g[u][2][e] + (g[u][3][e] - g[u][2][e]) * fr;
        s[e] = vt + (vb - vt) * fc;
      }
      *reinterpret_cast<f32x4*>(buf + (sq * kDfPx + (i ^ sq)) * 4) = s;
    }
  };

  f32x16 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
  const int mi = lane & 31, mh = lane >> 5;
  // packed weights: [tap][C / 8][C / 32][64 lanes][4] (deform_pack_weights); this wave's tiles are wave NT .. wave NT + NT - 1
  const f32x4* wimg = reinterpret_cast<const f32x4*>(p.wt) + (size_t)wave * NT * 64 + lane;

  gather(0);
  stage(0, lds);
  __syncthreads();
#pragma unroll 1
  for (int chunk = 0; chunk < NCHUNK; ++chunk) {
    const float* cur = lds + (chunk & 1) * SMP;
    const bool more = chunk + 1 < NCHUNK;
    if (more) gather(chunk + 1);
    const int n = chunk / NSL, sl = chunk - n * NSL;
    const f32x4* wc = wimg + (size_t)(n * (C / 8) + sl * (kDfKC / 8)) * (C / 32) * 64;
#pragma unroll
    for (int m = 0; m < kDfKC / 8; ++m) {
      const int q = 2 * m + mh;
      const f32x4 s = *reinterpret_cast<const f32x4*>(cur + (q * kDfPx + (mi ^ q)) * 4);
      f32x4 wv[NT];
#pragma unroll
      for (int t = 0; t < NT; ++t) wv[t] = wc[(size_t)(m * (C / 32) + t) * 64];
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(wv[t][e], s[e], acc[t], 0, 0, 0);
    }
    // (the other buffer was last read before the previous barrier)
    if (more) stage(chunk + 1, lds + ((chunk + 1) & 1) * SMP);
    __syncthreads();
  }

  // ---- D register r of lane l: output channel (r & 3) + 8 (r >> 2) + 4 (l >> 5) of the tile, pixel l & 31
  float vmax = 0.f;
  const int pix = pix0 + mi;
  if (pix < M) {
    float* orow = p.out + (pix * C + wave * NT * 32 + 4 * mh);
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int gq = 0; gq < 4; ++gq) {
        const f32x4 v = {acc[t][4 * gq], acc[t][4 * gq + 1], acc[t][4 * gq + 2], acc[t][4 * gq + 3]};
        *reinterpret_cast<f32x4*>(orow + t * 32 + 8 * gq) = v;
        vmax = fmaxf(vmax, fmaxf(fmaxf(fabsf(v[0]), fabsf(v[1])), fmaxf(fabsf(v[2]), fabsf(v[3]))));
      }
  }
  publish_amax_wg<256>(p.out_amax, vmax, tid, reinterpret_cast<unsigned char*>(lds));
}

}  // namespace

size_t deform_offset_weight_elems(int C) { return (size_t)9 * (C / 8) * 64 * 4; }
size_t deform_weight_elems(int C) { return (size_t)9 * C * C; }

// conv2_offset/W, HWIO [3][3][C][18] -> [tap][C / 8][64 lanes][4]: lane l, element e = w[tap][8 m + 4 (l >> 5) + e][l & 31]
// (rows 18 .. 31 of the MFMA tile are zero)
int deform_pack_offset_weights(const float* hwio, int C, float* dst) {
  ODT_CHECK(C == 128 || C == 256 || C == 512, "deformable conv: C must be 128, 256 or 512");
  for (int n = 0; n < 9; ++n)
    for (int m = 0; m < C / 8; ++m)
      for (int l = 0; l < 64; ++l)
        for (int e = 0; e < 4; ++e) {
          const int ci = 8 * m + 4 * (l >> 5) + e, j = l & 31;
          dst[(((size_t)n * (C / 8) + m) * 64 + l) * 4 + e] = j < 18 ? hwio[((size_t)n * C + ci) * 18 + j] : 0.f;
        }
  return 0;
}

// conv2/W, HWIO [3][3][C][C] -> [tap][C / 8][C / 32][64 lanes][4]: lane l, element e of tile t = w[tap][8 m + 4 (l >> 5) + e][32 t + (l & 31)]
int deform_pack_weights(const float* hwio, int C, float* dst) {
  ODT_CHECK(C == 128 || C == 256 || C == 512, "deformable conv: C must be 128, 256 or 512");
  for (int n = 0; n < 9; ++n)
    for (int m = 0; m < C / 8; ++m)
      for (int t = 0; t < C / 32; ++t)
        for (int l = 0; l < 64; ++l)
          for (int e = 0; e < 4; ++e) {
            const int ci = 8 * m + 4 * (l >> 5) + e, co = 32 * t + (l & 31);
            dst[((((size_t)n * (C / 8) + m) * (C / 32) + t) * 64 + l) * 4 + e] = hwio[((size_t)n * C + ci) * C + co];
          }
  return 0;
}

int launch_deform_conv(const DeformConvParams& p, hipStream_t stream, hipEvent_t between) {
  ODT_CHECK(p.in && p.wt_off && p.b_off && p.wt && p.off && p.out, "deformable conv: null argument");
  ODT_CHECK(p.C == 128 || p.C == 256 || p.C == 512, "deformable conv: C must be 128, 256 or 512");
  ODT_CHECK(p.B >= 1 && p.H >= 1 && p.W >= 1 && p.Ha >= p.H && p.Wa >= p.W && p.ldc >= p.C && p.ldc % 4 == 0,
            "deformable conv: bad geometry");
  ODT_CHECK(p.Ho == (p.H + 1) / 2 && p.Wo == (p.W + 1) / 2, "deformable conv: the output is [ceil(H / 2), ceil(W / 2)]");
  // (the kernels address the tensors with 32-bit element offsets)
  ODT_CHECK((double)p.B * p.Ha * p.Wa * p.ldc < 2147483648.0 && ((double)p.B * p.Ho * p.Wo + kDfPx) * p.C < 2147483648.0,
            "deformable conv: a tensor reaches 2^31 elements");
  const unsigned grid = (unsigned)((p.B * p.Ho * p.Wo + kDfPx - 1) / kDfPx);
  hipLaunchKernelGGL(deform_offset_kernel, dim3(grid), dim3(256), 0, stream, p);
  if (between != nullptr) ODT_HIP(hipEventRecord(between, stream));
  switch (p.C) {
    case 128: hipLaunchKernelGGL(deform_conv_kernel<1>, dim3(grid), dim3(256), 0, stream, p); break;
    case 256: hipLaunchKernelGGL(deform_conv_kernel<2>, dim3(grid), dim3(256), 0, stream, p); break;
    default: hipLaunchKernelGGL(deform_conv_kernel<4>, dim3(grid), dim3(256), 0, stream, p); break;
  }
  ODT_HIP(hipGetLastError());
  return 0;
}

}  // namespace odt
