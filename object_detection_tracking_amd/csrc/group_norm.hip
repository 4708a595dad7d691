// GroupNorm (--use_gn; reference nn.py:81-108: group_norm(x, group = 32), eps 1e-5) on NHWC f32.  Per image and per group of
// C / 32 adjacent channels, over all h * w positions: mean and the biased variance mean((x - mean)^2) as tf.nn.moments gives
// them, then tf.nn.batch_normalization: a = rsqrt(var + eps) * gamma[c], y = x * a + (beta[c] - mean * a).  The statistics
// come from the frame, so nothing can be folded into the conv weights: three launches behind the conv.
//   stats     one pass over the tensor with 16-byte loads: per (image, group) a sum and a sum of squares, accumulated in f64
//             (the square of an f32 is exact there, so E[x^2] - mean^2 is good to f32 rounding even at |mean| / std ~ 1000).
//             Fixed order, no float atomics: thread -> LDS -> per-group sums in index order -> one partial per workgroup in
//             part[B][32][parts][2].  The thread-to-channel map holds for any C % 32 == 0, so the step across threads goes
//             through LDS in index order rather than through wave shuffles.  The row ranges depend on the map alone, never
//             on B: an image gives the same bits at any position of a batch
//   finalize  grid (B): the partials of a group added in index order; mean and var rounded to f32 once; a[b][c] and
//             s[b][c] = beta[c] - mean * a[b][c] in f32 with the reference's operand order
//   apply     out = x * a + s (+ res | + res nearest-2x upsampled), optional ReLU; the output's |max| recorded for the next
//             convs' fp16x2 kernels (publish_amax_wg).  x, out and res each come with their own pitches; out's interior may
//             sit at an offset inside a tensor whose border is never written
// A thread keeps one channel quad -- its a / s sit in registers -- and walks the pixels of its rows: no division in the loops.
// Built with -ffp-contract=off: the apply step is one multiply and one (two) add(s), bit-identical to numpy f32.
#include "conv_split_epilogue.hpp"

namespace odt {
namespace {

constexpr int kGnThreads = 256;

// the workgroup's thread tile over (pixel, channel quad): the C / 4 quads of a pixel are cut into `qb` blocks of `tqn` quads
// (blockIdx.z), `tpn` pixels side by side; threads past tqn * tpn idle
struct GnTile { int qb, tqn, tpn; };
__host__ __device__ __forceinline__ GnTile gn_tile(int C) {
  GnTile t;
  const int c4n = C >> 2;
  t.qb = (c4n + kGnThreads - 1) / kGnThreads;
  t.tqn = (c4n + t.qb - 1) / t.qb;
  t.tpn = kGnThreads / t.tqn;
  return t;
}

// grid (chunks, B, qb): workgroup (k, b, z) sums rows [k * rpc, (k + 1) * rpc) of image b over the channels of quad block z
__global__ void __launch_bounds__(kGnThreads) group_norm_stats_kernel(GroupNormParams p) {
  __shared__ double red[2][kGnThreads][4];
  const int tid = threadIdx.x, b = blockIdx.y, z = blockIdx.z;
  const GnTile t = gn_tile(p.C);
  const int tp = tid / t.tqn, tq = tid - tp * t.tqn;
  const int q = z * t.tqn + tq;
  const bool active = tp < t.tpn && q < (p.C >> 2);
  const int rpc = (p.h + (int)gridDim.x - 1) / (int)gridDim.x;
  const int r0 = (int)blockIdx.x * rpc, r1 = r0 + rpc < p.h ? r0 + rpc : p.h;
  double s[4] = {0.0, 0.0, 0.0, 0.0}, ss[4] = {0.0, 0.0, 0.0, 0.0};
  if (active) {
    const float* xb = p.x + (long)b * p.Ha * p.Wa * p.ldc + q * 4;      // (launcher: an image stays below 2^30 elements)
    const int step = t.tpn * p.ldc;
    for (int y = r0; y < r1; ++y) {
      const float* row = xb + ((p.xoy + y) * p.Wa + p.xox) * p.ldc;
      int xx = tp;
      for (; xx + 3 * t.tpn < p.w; xx += 4 * t.tpn) {          // four 16-byte loads in flight
        const float* a = row + xx * p.ldc;
        const f32x4 v0 = *reinterpret_cast<const f32x4*>(a), v1 = *reinterpret_cast<const f32x4*>(a + step);
        const f32x4 v2 = *reinterpret_cast<const f32x4*>(a + 2 * step), v3 = *reinterpret_cast<const f32x4*>(a + 3 * step);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const double d0 = v0[e], d1 = v1[e], d2 = v2[e], d3 = v3[e];
          s[e] += d0; ss[e] += d0 * d0;
          s[e] += d1; ss[e] += d1 * d1;
          s[e] += d2; ss[e] += d2 * d2;
          s[e] += d3; ss[e] += d3 * d3;
        }
      }
      for (; xx < p.w; xx += t.tpn) {
        const f32x4 v0 = *reinterpret_cast<const f32x4*>(row + xx * p.ldc);
#pragma unroll
        for (int e = 0; e < 4; ++e) { const double d0 = v0[e]; s[e] += d0; ss[e] += d0 * d0; }
      }
    }
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) { red[0][tid][e] = s[e]; red[1][tid][e] = ss[e]; }
  __syncthreads();
  if (tid < kGnGroups) {
    // group tid: its channels inside this quad block, in channel order; per channel the pixel threads in index order.  A
    // workgroup whose block holds none of them writes zeros (adding +0.0 changes nothing)
    const int cg = p.C / kGnGroups;
    const int clo = z * t.tqn * 4, chi = (z + 1) * t.tqn * 4 < p.C ? (z + 1) * t.tqn * 4 : p.C;
    const int c0 = tid * cg > clo ? tid * cg : clo, c1 = (tid + 1) * cg < chi ? (tid + 1) * cg : chi;
    double S = 0.0, SS = 0.0;
    for (int c = c0; c < c1; ++c) {
      const int ql = (c >> 2) - z * t.tqn, e = c & 3;
      for (int k = 0; k < t.tpn; ++k) { S += red[0][k * t.tqn + ql][e]; SS += red[1][k * t.tqn + ql][e]; }
    }
    const long nparts = (long)gridDim.x * gridDim.z;
    double* dst = p.part + (((long)b * kGnGroups + tid) * nparts + (long)blockIdx.x * gridDim.z + z) * 2;
    dst[0] = S; dst[1] = SS;
  }
}

// grid (B): mean / var of the image's 32 groups, then a and s of its C channels
__global__ void __launch_bounds__(kGnThreads) group_norm_finalize_kernel(GroupNormParams p, int nparts) {
  __shared__ float mv[2][kGnGroups];
  const int tid = threadIdx.x, b = blockIdx.x;
  const int cg = p.C / kGnGroups;
  if (tid < kGnGroups) {
    const double* src = p.part + ((long)b * kGnGroups + tid) * nparts * 2;
    double S = 0.0, SS = 0.0;
    for (int i = 0; i < nparts; ++i) { S += src[2 * i]; SS += src[2 * i + 1]; }
    const double n = (double)p.h * (double)p.w * (double)cg;
    const double mu = S / n;
    double v = SS / n - mu * mu;
    v = v > 0.0 ? v : 0.0;
    const float mean = (float)mu, var = (float)v;
    mv[0][tid] = mean; mv[1][tid] = var;
    p.mean[b * kGnGroups + tid] = mean; p.var[b * kGnGroups + tid] = var;
  }
  __syncthreads();
  float* a_row = p.ab + (long)b * 2 * p.C;
  for (int c = tid; c < p.C; c += kGnThreads) {
    const int g = c / cg;
    const float a = (1.0f / sqrtf(mv[1][g] + p.eps)) * p.gamma[c];
    a_row[c] = a;
    a_row[p.C + c] = p.beta[c] - mv[0][g] * a;
  }
}

template <int RES>
__device__ __forceinline__ void gn_store(float* dst, f32x4 v, f32x4 r, f32x4 a, f32x4 s, int relu, float& vmax) {
  v = v * a;
  v = v + s;
  if (RES != 0) v = v + r;
  if (relu) {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
  }
  *reinterpret_cast<f32x4*>(dst) = v;
  vmax = fmaxf(vmax, fmaxf(fmaxf(fabsf(v[0]), fabsf(v[1])), fmaxf(fabsf(v[2]), fabsf(v[3]))));
}

// grid (row workgroups, B, qb): a workgroup takes every gridDim.x-th row of its image; two pixels per thread and pass, all
// their loads issued before the first store.  RES: 0 none | 1 same shape | 2 nearest-2x upsample of [B, res_H, res_W, *]
template <int RES>
__global__ void __launch_bounds__(kGnThreads) group_norm_apply_kernel(GroupNormParams p) {
  __shared__ float red[kGnThreads / 64];
  const int tid = threadIdx.x, b = blockIdx.y, z = blockIdx.z;
  const GnTile t = gn_tile(p.C);
  const int tp = tid / t.tqn, tq = tid - tp * t.tqn;
  const int q = z * t.tqn + tq;
  const bool active = tp < t.tpn && q < (p.C >> 2);
  float vmax = 0.f;
  if (active) {
    const float* ab = p.ab + (long)b * 2 * p.C + q * 4;
    const f32x4 a = *reinterpret_cast<const f32x4*>(ab), s = *reinterpret_cast<const f32x4*>(ab + p.C);
    const float* xb = p.x + (long)b * p.Ha * p.Wa * p.ldc + q * 4;
    float* ob = p.out + (long)b * p.oH * p.oW * p.out_ldc + q * 4;
    const float* rb = RES != 0 ? p.res + (long)b * p.res_H * p.res_W * p.res_ldc + q * 4 : nullptr;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    for (int y = (int)blockIdx.x; y < p.h; y += (int)gridDim.x) {
      const float* xrow = xb + ((p.xoy + y) * p.Wa + p.xox) * p.ldc;
      float* orow = ob + ((p.oy + y) * p.oW + p.ox) * p.out_ldc;
      const float* rrow = RES == 1 ? rb + y * p.res_W * p.res_ldc : (RES == 2 ? rb + (y >> 1) * p.res_W * p.res_ldc : nullptr);
      int xx = tp;
      for (; xx + t.tpn < p.w; xx += 2 * t.tpn) {
        const int x1 = xx + t.tpn;
        const f32x4 v0 = *reinterpret_cast<const f32x4*>(xrow + xx * p.ldc), v1 = *reinterpret_cast<const f32x4*>(xrow + x1 * p.ldc);
        f32x4 g0 = zero, g1 = zero;
        if (RES == 1) {
          g0 = *reinterpret_cast<const f32x4*>(rrow + xx * p.res_ldc); g1 = *reinterpret_cast<const f32x4*>(rrow + x1 * p.res_ldc);
        } else if (RES == 2) {
          g0 = *reinterpret_cast<const f32x4*>(rrow + (xx >> 1) * p.res_ldc); g1 = *reinterpret_cast<const f32x4*>(rrow + (x1 >> 1) * p.res_ldc);
        }
        gn_store<RES>(orow + xx * p.out_ldc, v0, g0, a, s, p.relu, vmax);
        gn_store<RES>(orow + x1 * p.out_ldc, v1, g1, a, s, p.relu, vmax);
      }
      if (xx < p.w) {
        const f32x4 v0 = *reinterpret_cast<const f32x4*>(xrow + xx * p.ldc);
        f32x4 g0 = zero;
        if (RES == 1) g0 = *reinterpret_cast<const f32x4*>(rrow + xx * p.res_ldc);
        else if (RES == 2) g0 = *reinterpret_cast<const f32x4*>(rrow + (xx >> 1) * p.res_ldc);
        gn_store<RES>(orow + xx * p.out_ldc, v0, g0, a, s, p.relu, vmax);
      }
    }
  }
  publish_amax_wg<kGnThreads>(p.amax, vmax, tid, reinterpret_cast<unsigned char*>(red));
}

}  // namespace

int group_norm_chunks(int h, int w, int C) {
  const long quads = (long)h * w * (C / 4);
  return (int)std::max<long>(1, std::min<long>((quads + 4095) / 4096, std::min(h, 256)));
}

int group_norm_parts(int h, int w, int C, int chunks) {
  return (chunks > 0 ? chunks : group_norm_chunks(h, w, C)) * gn_tile(C).qb;
}

int launch_group_norm(const GroupNormParams& p, hipStream_t stream) {
  ODT_CHECK(p.x && p.gamma && p.beta && p.out && p.part && p.ab && p.mean && p.var, "group_norm: null argument");
  ODT_CHECK(p.B >= 1 && p.B <= 65535 && p.h >= 1 && p.w >= 1, "group_norm: bad sizes");
  ODT_CHECK(p.C >= kGnGroups && p.C % kGnGroups == 0, "group_norm: C must be a multiple of 32 (32 groups)");
  ODT_CHECK(p.ldc % 4 == 0 && p.out_ldc % 4 == 0 && p.ldc >= p.C && p.out_ldc >= p.C,
            "group_norm: a pixel stride (ldc) must be a multiple of 4 and hold the C channels");
  ODT_CHECK(p.xoy >= 0 && p.xox >= 0 && p.xoy + p.h <= p.Ha && p.xox + p.w <= p.Wa, "group_norm: the view of x lies outside its allocation");
  ODT_CHECK(p.oy >= 0 && p.ox >= 0 && p.oy + p.h <= p.oH && p.ox + p.w <= p.oW, "group_norm: the view of out lies outside its allocation");
  // (32-bit element offsets inside an image)
  ODT_CHECK((double)p.Ha * p.Wa * p.ldc < 1073741824.0 && (double)p.oH * p.oW * p.out_ldc < 1073741824.0,
            "group_norm: an image of the tensor reaches 2^30 elements");
  ODT_CHECK(p.res_mode >= 0 && p.res_mode <= 2 && (p.res_mode == 0 || p.res != nullptr), "group_norm: bad residual mode");
  if (p.res_mode != 0) {
    ODT_CHECK(p.res_ldc % 4 == 0 && p.res_ldc >= p.C, "group_norm: the residual's pixel stride must be a multiple of 4 and hold the C channels");
    ODT_CHECK(p.res_mode == 1 ? (p.res_H >= p.h && p.res_W >= p.w) : (p.res_H * 2 >= p.h && p.res_W * 2 >= p.w),
              "group_norm: the residual is smaller than the view");
    ODT_CHECK((double)p.res_H * p.res_W * p.res_ldc < 1073741824.0, "group_norm: an image of the residual reaches 2^30 elements");
  }
  ODT_CHECK(p.chunks >= 0 && p.chunks <= p.h && p.chunks <= 65535, "group_norm: chunks must lie in [0, h]");
  const int chunks = p.chunks > 0 ? p.chunks : group_norm_chunks(p.h, p.w, p.C);
  const GnTile t = gn_tile(p.C);
  hipLaunchKernelGGL(group_norm_stats_kernel, dim3(chunks, p.B, t.qb), dim3(kGnThreads), 0, stream, p);
  hipLaunchKernelGGL(group_norm_finalize_kernel, dim3(p.B), dim3(kGnThreads), 0, stream, p, chunks * t.qb);
  // about 2048 workgroups in all
  const int gx = std::max(1, std::min(p.h, 2048 / (p.B * t.qb)));
  const dim3 grid(gx, p.B, t.qb);
  if (p.res_mode == 0) hipLaunchKernelGGL(group_norm_apply_kernel<0>, grid, dim3(kGnThreads), 0, stream, p);
  else if (p.res_mode == 1) hipLaunchKernelGGL(group_norm_apply_kernel<1>, grid, dim3(kGnThreads), 0, stream, p);
  else hipLaunchKernelGGL(group_norm_apply_kernel<2>, grid, dim3(kGnThreads), 0, stream, p);
  ODT_HIP(hipGetLastError());
  return 0;
}

}  // namespace odt
