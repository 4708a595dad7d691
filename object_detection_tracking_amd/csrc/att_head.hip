// The attention branch of the box head (--use_att_frcnn_head; reference fastrcnn_2fc_head, models.py:1064-1089) on f32, the same
// in every arithmetic mode.  The reference's attention map is conv2d(feature, 1 channel, activation = softmax): a softmax over
// an axis of ONE channel, which is exactly 1.0f for every finite logit -- so `attended` is the plain sum of the RoI's 49
// positions and fastrcnn/attention/{W,b} cannot reach the output.  Two bandwidth-bound kernels; the
// dense layer between them (att_trans) runs on the conv kernels.
//   att_pool  x [R, 49, C] (the box head's RoI features, dense, C % 4 == 0) -> out [R, C]: one thread owns a channel quad of one
//             RoI and adds its 49 positions to +0 one after another, in row-major (h, w) order, in f32.  Loads are 16 bytes,
//             adjacent threads read adjacent quads, seven loads are in flight per thread.  No float atomics and nothing depends
//             on R or on the RoI's row: a RoI gives the same bits at any row of any batch.  A zero RoI (a row past an image's
//             proposal count) sums to zeros like any other
//   att_add   out [R, D] = h [R, D at row pitch ldh] + a [R, D], D % 4 == 0, 16-byte loads and stores, four quads per thread: the
//             reference's hidden + relu(att_trans) -- the add sits BEHIND the ReLU, which a conv epilogue's relu(acc + b + res)
//             is not
// Both record the |max| of what they store in a range slot (publish_amax_wg), as roi_align_kernel and group_norm_roi_kernel do,
// so that att_trans and fastrcnn/outputs stay on the fp16x2 kernels.
#include "conv_split_epilogue.hpp"

namespace odt {
namespace {

constexpr int kAttThreads = 256;
constexpr int kAttPos = 49;          // 7 x 7 positions of a RoI
constexpr int kAttBatch = 7;         // loads a thread issues before it adds them (a row of the RoI)
constexpr int kAttAddQuads = 4;      // quads a thread of att_add_kernel owns, 256 quads apart

__device__ __forceinline__ float quad_amax(const f32x4& y) {
  return fmaxf(fmaxf(fabsf(y[0]), fabsf(y[1])), fmaxf(fabsf(y[2]), fabsf(y[3])));
}

__global__ void __launch_bounds__(kAttThreads) att_pool_kernel(AttPoolParams p) {
  __shared__ float red[kAttThreads / 64];
  const int tid = threadIdx.x, q4 = p.C >> 2;
  const long i = (long)blockIdx.x * kAttThreads + tid;      // (RoI, channel quad)
  float vmax = 0.f;
  if (i < (long)p.R * q4) {
    const long r = i / q4;
    const int q = (int)(i - r * q4);
    const float* xb = p.x + (size_t)r * kAttPos * p.C + q * 4;
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
    for (int k0 = 0; k0 < kAttPos; k0 += kAttBatch) {
      f32x4 v[kAttBatch];
#pragma unroll
      for (int k = 0; k < kAttBatch; ++k) v[k] = *reinterpret_cast<const f32x4*>(xb + (size_t)(k0 + k) * p.C);
#pragma unroll
      for (int k = 0; k < kAttBatch; ++k) s = s + v[k];
    }
    *reinterpret_cast<f32x4*>(p.out + (size_t)r * p.C + q * 4) = s;
    vmax = quad_amax(s);
  }
  publish_amax_wg<kAttThreads>(p.amax, vmax, tid, reinterpret_cast<unsigned char*>(red));
}

__global__ void __launch_bounds__(kAttThreads) att_add_kernel(AttAddParams p) {
  __shared__ float red[kAttThreads / 64];
  const int tid = threadIdx.x, q4 = p.D >> 2;
  const int n = p.R * q4, i0 = (int)blockIdx.x * (kAttThreads * kAttAddQuads) + tid;      // (R * ldh < 2^31: launch_att_add)
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  // quads i0, i0 + 256, ... of the flattened (row, quad) index: the eight loads are issued before the first add
  f32x4 h[kAttAddQuads], a[kAttAddQuads];
  int r[kAttAddQuads], q[kAttAddQuads];
#pragma unroll
  for (int j = 0; j < kAttAddQuads; ++j) {
    const int i = i0 + j * kAttThreads;
    r[j] = i / q4; q[j] = i - r[j] * q4;
    const bool ok = i < n;
    h[j] = ok ? *reinterpret_cast<const f32x4*>(p.h + (size_t)r[j] * p.ldh + q[j] * 4) : zero;
    a[j] = ok ? *reinterpret_cast<const f32x4*>(p.a + (size_t)r[j] * p.D + q[j] * 4) : zero;
  }
  float vmax = 0.f;
#pragma unroll
  for (int j = 0; j < kAttAddQuads; ++j) {
    if (i0 + j * kAttThreads >= n) continue;
    const f32x4 y = h[j] + a[j];
    *reinterpret_cast<f32x4*>(p.out + (size_t)r[j] * p.D + q[j] * 4) = y;
    vmax = fmaxf(vmax, quad_amax(y));
  }
  publish_amax_wg<kAttThreads>(p.amax, vmax, tid, reinterpret_cast<unsigned char*>(red));
}

}  // namespace

static_assert(kAttPos % kAttBatch == 0, "att_pool_kernel adds whole batches of positions");

int launch_att_pool(const AttPoolParams& p, hipStream_t stream) {
  ODT_CHECK(p.x && p.out, "att_pool: null argument");
  ODT_CHECK(p.R >= 1 && p.C >= 1, "att_pool: bad sizes");
  ODT_CHECK(p.C % 4 == 0, "att_pool: C must be a multiple of 4 (a thread owns a channel quad)");
  ODT_CHECK((double)p.R * kAttPos * p.C < 2147483648.0, "att_pool: the RoI tensor is too large");
  ODT_CHECK((((uintptr_t)p.x | (uintptr_t)p.out) & 15) == 0, "att_pool: x and out must be 16-byte aligned");
  const long n = (long)p.R * (p.C >> 2);
  hipLaunchKernelGGL(att_pool_kernel, dim3((unsigned)((n + kAttThreads - 1) / kAttThreads)), dim3(kAttThreads), 0, stream, p);
  ODT_HIP(hipGetLastError());
  return 0;
}

int launch_att_add(const AttAddParams& p, hipStream_t stream) {
  ODT_CHECK(p.h && p.a && p.out, "att_add: null argument");
  ODT_CHECK(p.R >= 1 && p.D >= 1, "att_add: bad sizes");
  ODT_CHECK(p.D % 4 == 0, "att_add: D must be a multiple of 4 (a thread owns a quad)");
  ODT_CHECK(p.ldh >= p.D && p.ldh % 4 == 0, "att_add: the row pitch of h (ldh) must be a multiple of 4 and hold the D columns");
  ODT_CHECK((double)p.R * p.ldh < 2147483648.0, "att_add: the tensors are too large");
  ODT_CHECK((((uintptr_t)p.h | (uintptr_t)p.a | (uintptr_t)p.out) & 15) == 0, "att_add: h, a and out must be 16-byte aligned");
  const long n = (long)p.R * (p.D >> 2), per = (long)kAttThreads * kAttAddQuads;
  hipLaunchKernelGGL(att_add_kernel, dim3((unsigned)((n + per - 1) / per)), dim3(kAttThreads), 0, stream, p);
  ODT_HIP(hipGetLastError());
  return 0;
}

}  // namespace odt
