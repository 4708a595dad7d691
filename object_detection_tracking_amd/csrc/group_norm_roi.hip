// GroupNorm of ROI tensors (--use_gn with --use_conv_frcnn_head; reference nn.py:81-108 behind each conv of conv_frcnn_head,
// models.py:1110-1124) on NHWC f32: x is [R, hw, ldc] with R = B K "images" of hw <= 64 pixels (7 x 7 in the plans).  The
// frame kernels (group_norm.hip) make three passes with one image per blockIdx.y; here a ROI's share of a workgroup fits
// its registers, so the layer is ONE launch and ONE pass: load, reduce, apply from the registers, store.
//   split     grid (R, qb): the C / 4 channel quads of a ROI are cut into qb = ceil(C / 256) blocks of tqn quads -- whole groups,
//             32 / qb of them (gn_roi_tile) -- and tpn = 256 / tqn threads stand side by side over the pixels: thread (tp, tq)
//             keeps pixels tp, tp + tpn, ... of quad tq, at most kGnRoiQuads 16-byte loads, all issued before the first use.
//             Threads past tqn * tpn and pixels past hw load nothing
//   reduce    per thread and channel a sum and a sum of squares in f64 (the square of an f32 is exact there), pixel order;
//             through LDS to one thread per group, which adds its channels in channel order and, per channel, the pixel
//             threads in index order.  No float atomics, and nothing depends on R or on the ROI's row: a ROI gives the same
//             bits at any row and in any batch
//   apply     the arithmetic of group_norm.hip: mean and var = max(E[x^2] - mean^2, 0) rounded to f32 once, a = (1 / sqrtf(var
//             + eps)) * gamma[c], s = beta[c] - mean * a, out = x * a + s: one multiply and one add (-ffp-contract=off).  The
//             output's |max| goes to the range slot (publish_amax_wg) for the next conv's fp16x2 kernel
#include "conv_split_epilogue.hpp"

namespace odt {
namespace {

constexpr int kGnRoiThreads = 256;
constexpr int kGnRoiMaxHw = 64;
constexpr int kGnRoiMaxC = 512;
constexpr int kGnRoiQuads = 16;      // quads a thread keeps: ceil(64 / tpn) at the smallest tpn (4, where tqn = 64)

// the workgroup's thread tile: qb channel blocks (blockIdx.y) of tqn quads = 32 / qb whole groups, tpn pixel threads per quad
struct GnRoiTile { int qb, tqn, tpn; };
__host__ __device__ __forceinline__ GnRoiTile gn_roi_tile(int C) {
  GnRoiTile t;
  t.qb = (C + 255) / 256;            // 1 or 2 for C <= 512; C % 32 == 0 makes C / qb a multiple of 16 channels
  t.tqn = (C >> 2) / t.qb;           // 8 .. 64
  t.tpn = kGnRoiThreads / t.tqn;     // 4 .. 32
  return t;
}

__global__ void __launch_bounds__(kGnRoiThreads) group_norm_roi_kernel(RoiGroupNormParams p) {
  __shared__ double red[2][4][kGnRoiThreads];      // [sum | sum of squares][element of the quad][thread]
  __shared__ float mv[2][kGnGroups];
  const int tid = threadIdx.x, z = blockIdx.y;
  const long r = blockIdx.x;
  const GnRoiTile t = gn_roi_tile(p.C);
  const int tp = tid / t.tqn, tq = tid - tp * t.tqn;
  const bool active = tp < t.tpn;
  const int c0 = (z * t.tqn + tq) * 4;              // the thread's first channel
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  f32x4 v[kGnRoiQuads];
  if (active) {
    const float* xb = p.x + r * p.hw * p.ldc + c0;
#pragma unroll
    for (int i = 0; i < kGnRoiQuads; ++i) {
      const int px = tp + i * t.tpn;
      v[i] = px < p.hw ? *reinterpret_cast<const f32x4*>(xb + px * p.ldc) : zero;
    }
    double s[4] = {0.0, 0.0, 0.0, 0.0}, ss[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int i = 0; i < kGnRoiQuads; ++i) {          // (a pixel past hw adds +0.0: nothing changes)
#pragma unroll
      for (int e = 0; e < 4; ++e) { const double d = v[i][e]; s[e] += d; ss[e] += d * d; }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) { red[0][e][tid] = s[e]; red[1][e][tid] = ss[e]; }
  }
  __syncthreads();
  const int cg = p.C / kGnGroups, gpb = kGnGroups / t.qb;      // channels per group, groups per channel block
  if (tid < gpb) {
    // group z * gpb + tid: its channels in channel order; per channel the pixel threads in index order
    const int cl0 = tid * cg;                        // first channel of the group inside this block
    double S = 0.0, SS = 0.0;
    for (int c = cl0; c < cl0 + cg; ++c) {
      const int ql = c >> 2, e = c & 3;
      for (int k = 0; k < t.tpn; ++k) { S += red[0][e][k * t.tqn + ql]; SS += red[1][e][k * t.tqn + ql]; }
    }
    const double n = (double)p.hw * (double)cg;
    const double mu = S / n;
    double var = SS / n - mu * mu;
    var = var > 0.0 ? var : 0.0;
    const float mean = (float)mu, varf = (float)var;
    mv[0][tid] = mean; mv[1][tid] = varf;
    if (p.mean != nullptr) p.mean[r * kGnGroups + z * gpb + tid] = mean;
    if (p.var != nullptr) p.var[r * kGnGroups + z * gpb + tid] = varf;
  }
  __syncthreads();
  float vmax = 0.f;
  if (active) {
    const f32x4 gm = *reinterpret_cast<const f32x4*>(p.gamma + c0), bt = *reinterpret_cast<const f32x4*>(p.beta + c0);
    f32x4 a, s;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int g = (tq * 4 + e) / cg;               // the group inside this block (a quad spans several where cg < 4)
      const float ae = (1.0f / sqrtf(mv[1][g] + p.eps)) * gm[e];
      a[e] = ae;
      s[e] = bt[e] - mv[0][g] * ae;
    }
    float* ob = p.out + r * p.hw * p.out_ldc + c0;
#pragma unroll
    for (int i = 0; i < kGnRoiQuads; ++i) {
      const int px = tp + i * t.tpn;
      if (px < p.hw) {
        f32x4 y = v[i] * a;
        y = y + s;
        *reinterpret_cast<f32x4*>(ob + px * p.out_ldc) = y;
        vmax = fmaxf(vmax, fmaxf(fmaxf(fabsf(y[0]), fabsf(y[1])), fmaxf(fabsf(y[2]), fabsf(y[3]))));
      }
    }
  }
  publish_amax_wg<kGnRoiThreads>(p.amax, vmax, tid, reinterpret_cast<unsigned char*>(red));
}

}  // namespace

int launch_group_norm_roi(const RoiGroupNormParams& p, hipStream_t stream) {
  ODT_CHECK(p.x && p.gamma && p.beta && p.out, "group_norm_roi: null argument");
  ODT_CHECK(p.R >= 1 && p.hw >= 1, "group_norm_roi: bad sizes");
  ODT_CHECK(p.hw <= kGnRoiMaxHw, "group_norm_roi: a ROI holds at most 64 pixels (h * w <= 64)");
  ODT_CHECK(p.C >= kGnGroups && p.C <= kGnRoiMaxC && p.C % kGnGroups == 0,
            "group_norm_roi: C must be a multiple of 32 (32 groups) in [32, 512]");
  ODT_CHECK(p.ldc % 4 == 0 && p.out_ldc % 4 == 0 && p.ldc >= p.C && p.out_ldc >= p.C,
            "group_norm_roi: a pixel stride (ldc) must be a multiple of 4 and hold the C channels");
  ODT_CHECK(p.ldc <= (1 << 20) && p.out_ldc <= (1 << 20), "group_norm_roi: a pixel stride (ldc) is too large");      // (32-bit offsets inside a ROI)
  ODT_CHECK((((uintptr_t)p.x | (uintptr_t)p.out | (uintptr_t)p.gamma | (uintptr_t)p.beta) & 15) == 0,
            "group_norm_roi: x, out, gamma and beta must be 16-byte aligned");
  const GnRoiTile t = gn_roi_tile(p.C);
  // (what the kernel's register tile and its whole-group channel blocks rest on)
  ODT_CHECK(t.tqn * t.qb * 4 == p.C && kGnGroups % t.qb == 0 && t.tqn <= 64 && t.tpn >= 1 &&
            (kGnRoiMaxHw + t.tpn - 1) / t.tpn <= kGnRoiQuads, "group_norm_roi: no thread tile for this C");
  hipLaunchKernelGGL(group_norm_roi_kernel, dim3((unsigned)p.R, (unsigned)t.qb), dim3(kGnRoiThreads), 0, stream, p);
  ODT_HIP(hipGetLastError());
  return 0;
}

}  // namespace odt
