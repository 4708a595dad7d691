// Squeeze-excitation for the ResNet bottleneck (model version 6; reference nn.py:506-517): after conv3 + BN
//   squeeze = sigmoid(relu(mean_HW(l) . fc1/W + fc1/b) . fc2/W + fc2/b);  l = l * squeeze[:, :, None, None]
// and then the residual add + ReLU of every block.  conv3 is 1x1 and BN is affine, so the spatial mean commutes with them:
// the plan folds conv3 . BN into fc1 on the host and pools t2, conv2's ch-wide output, instead of the 4 ch-wide l -- a quarter
// of the bytes, and the gate does not wait for conv3.  Three pieces:
//   pool   launch_channel_mean (effnet.hip): per-(image, channel) sums in a fixed order, no float atomics
//   gate   two small launches: ch -> ch / 4 (ReLU) -> 4 ch (sigmoid) per image, fixed summation orders
//   apply  out = max(y * gate[b, c] + shortcut, 0) on NHWC f32: the one pass over the block's widest tensor that SE adds
//          (two reads, one write), with the output's |max| recorded for the next block's fp16x2 convs
// Built with -ffp-contract=off: the apply step is one multiply, one add, one max -- bit-identical to numpy f32.
#include "conv_split_epilogue.hpp"

namespace odt {
namespace {

constexpr int kRseMaxCh = 2048, kRseMaxR = 512;     // LDS staging of the mean / the reduced vector (R101: 512 / 128)

// stage A, grid (ceil(r / 4), B): one reduced channel per wave: rvec[j] = relu(b1[j] + <mean, w1[j]>), 64-lane strided
// partial sums + a fixed shuffle tree
__global__ void __launch_bounds__(256) resnet_se_reduce_kernel(ResSeParams p) {
  __shared__ float mean[kRseMaxCh];
  const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int c = tid; c < p.ch; c += 256) mean[c] = p.mean[(long)b * p.ch + c];
  __syncthreads();
  const int j = blockIdx.x * 4 + wave;
  if (j < p.r) {
    const float* w = p.w1 + (long)j * p.ch;
    float s = 0.f;
#pragma unroll 4
    for (int c = lane; c < p.ch; c += 64) s += mean[c] * w[c];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    if (lane == 0) p.rvec[(long)b * p.r + j] = fmaxf(s + p.b1[j], 0.f);
  }
}

// stage B, grid (ceil(cout / 256), B): gate[c] = sigmoid(b2[c] + sum_j rvec[j] * w2t[j][c]), j in index order
__global__ void __launch_bounds__(256) resnet_se_expand_kernel(ResSeParams p) {
  __shared__ float r[kRseMaxR];
  const int b = blockIdx.y, tid = threadIdx.x;
  for (int j = tid; j < p.r; j += 256) r[j] = p.rvec[(long)b * p.r + j];
  __syncthreads();
  const int c = blockIdx.x * 256 + tid;
  if (c >= p.cout) return;
  float s = p.b2[c];
#pragma unroll 8
  for (int j = 0; j < p.r; ++j) s += r[j] * p.w2t[(long)j * p.cout + c];
  p.gate[(long)b * p.gate_ld + c] = 1.0f / (1.0f + expf(-s));
}

// one channel quad of one pixel: nv valid channels (4, or fewer in the last quad of a pixel whose C is not a multiple of
// 4: the pad channels are read -- they lie inside the pixel's ldc -- but neither stored nor counted in the |max|)
__device__ __forceinline__ void rse_store(float* dst, f32x4 yv, f32x4 sv, f32x4 g, int nv, float& vmax) {
  f32x4 v = yv * g;
  v = v + sv;
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
  if (nv == 4) {
    *reinterpret_cast<f32x4*>(dst) = v;
    vmax = fmaxf(vmax, fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3])));
  } else {
#pragma unroll
    for (int e = 0; e < 3; ++e)
      if (e < nv) { dst[e] = v[e]; vmax = fmaxf(vmax, v[e]); }
  }
}

// grid (blocks per image, B).  A thread walks the (pixel, channel quad) pairs of its image with the stride of the image's
// workgroups; where that stride is a multiple of the quads per pixel (the launcher arranges it) the thread's channel quad --
// and with it its four gate values -- never changes: they sit in registers, and the loop has no division.  Two pairs per
// iteration, all four 16-byte loads issued before the first store.
__global__ void __launch_bounds__(256) resnet_se_apply_kernel(ResSeApplyParams p) {
  __shared__ float red[4];
  const int tid = threadIdx.x, b = blockIdx.y;
  const int c4n = (p.C + 3) >> 2;
  const int total = p.HW * c4n;                        // (launcher: HW * ldc < 2^30)
  const int step = (int)gridDim.x * 256;
  const long base = (long)b * p.HW * p.ldc;
  const float* y = p.y + base;
  const float* sc = p.sc + base;
  float* out = p.out + base;
  const float* grow = p.gate + (long)b * p.gate_ld;
  float vmax = 0.f;
  int i = (int)blockIdx.x * 256 + tid;
  if (step % c4n == 0) {
    if (i < total) {
      const int pix0 = i / c4n, c4 = i - pix0 * c4n;
      const int nv = p.C - c4 * 4 < 4 ? p.C - c4 * 4 : 4;
      const f32x4 g = *reinterpret_cast<const f32x4*>(grow + c4 * 4);
      const int ostep = (step / c4n) * p.ldc;
      const int oend = p.HW * p.ldc;
      int o = pix0 * p.ldc + c4 * 4;
      for (; o + ostep < oend; o += 2 * ostep) {
        const f32x4 y0 = *reinterpret_cast<const f32x4*>(y + o), y1 = *reinterpret_cast<const f32x4*>(y + o + ostep);
        const f32x4 s0 = *reinterpret_cast<const f32x4*>(sc + o), s1 = *reinterpret_cast<const f32x4*>(sc + o + ostep);
        rse_store(out + o, y0, s0, g, nv, vmax);
        rse_store(out + o + ostep, y1, s1, g, nv, vmax);
      }
      if (o < oend) {
        const f32x4 y0 = *reinterpret_cast<const f32x4*>(y + o);
        const f32x4 s0 = *reinterpret_cast<const f32x4*>(sc + o);
        rse_store(out + o, y0, s0, g, nv, vmax);
      }
    }
  } else {
    for (; i < total; i += step) {
      const int pix = i / c4n, c4 = i - pix * c4n;
      const int nv = p.C - c4 * 4 < 4 ? p.C - c4 * 4 : 4;
      const int o = pix * p.ldc + c4 * 4;
      const f32x4 g = *reinterpret_cast<const f32x4*>(grow + c4 * 4);
      const f32x4 y0 = *reinterpret_cast<const f32x4*>(y + o);
      const f32x4 s0 = *reinterpret_cast<const f32x4*>(sc + o);
      rse_store(out + o, y0, s0, g, nv, vmax);
    }
  }
  publish_amax_wg<256>(p.amax, vmax, tid, reinterpret_cast<unsigned char*>(red));
}

int rse_gcd(int a, int b) { while (b) { const int t = a % b; a = b; b = t; } return a; }

}  // namespace

static int rse_check_gate(const ResSeParams& p) {
  ODT_CHECK(p.B >= 1 && p.B <= 65535 && p.ch >= 1 && p.r >= 1 && p.cout >= 1 && p.gate_ld >= p.cout, "resnet_se: bad gate sizes");
  ODT_CHECK(p.ch <= kRseMaxCh && p.r <= kRseMaxR, "resnet_se: gate sizes outside the LDS staging");
  ODT_CHECK(p.mean && p.w1 && p.b1 && p.w2t && p.b2 && p.rvec && p.gate, "resnet_se: null gate argument");
  return 0;
}

int launch_resnet_se_mlp(const ResSeParams& p, hipStream_t stream) {
  if (rse_check_gate(p)) return 1;
  hipLaunchKernelGGL(resnet_se_reduce_kernel, dim3((p.r + 3) / 4, p.B), dim3(256), 0, stream, p);
  hipLaunchKernelGGL(resnet_se_expand_kernel, dim3((p.cout + 255) / 256, p.B), dim3(256), 0, stream, p);
  ODT_HIP(hipGetLastError());
  return 0;
}

int launch_resnet_se_gate(const ResSeParams& p, hipStream_t stream) {
  ODT_CHECK(p.t2 != nullptr && p.part != nullptr && p.HW >= 1 && p.ch % 4 == 0, "resnet_se: bad pool arguments");
  if (rse_check_gate(p)) return 1;
  if (launch_channel_mean(p.t2, p.B, p.HW, p.ch, p.part, p.mean, stream)) return 1;
  return launch_resnet_se_mlp(p, stream);
}

int launch_resnet_se_apply(const ResSeApplyParams& p, hipStream_t stream) {
  ODT_CHECK(p.y && p.sc && p.gate && p.out, "resnet_se_apply: null argument");
  ODT_CHECK(p.B >= 1 && p.B <= 65535 && p.HW >= 1 && p.C >= 1 && p.C <= p.ldc && p.ldc % 4 == 0 && p.gate_ld % 4 == 0 &&
            p.gate_ld >= (p.C + 3) / 4 * 4, "resnet_se_apply: bad sizes");
  // (32-bit element offsets inside an image; the walk may step once past the end before it stops)
  ODT_CHECK((double)p.HW * p.ldc < 1073741824.0, "resnet_se_apply: an image of the tensor reaches 2^30 elements");
  const int c4n = (p.C + 3) / 4;
  const long total = (long)p.HW * c4n;
  // two (pixel, quad) pairs per thread and pass, about 2048 workgroups in all; a whole number of pixels per stride
  long gx = std::min<long>((total + 511) / 512, std::max<long>(1, 2048 / p.B));
  const int m = c4n / rse_gcd(c4n, 256);
  if (gx >= m) gx = gx / m * m;
  hipLaunchKernelGGL(resnet_se_apply_kernel, dim3((unsigned)gx, p.B), dim3(256), 0, stream, p);
  ODT_HIP(hipGetLastError());
  return 0;
}

}  // namespace odt
