// Relation modules of the box head (--add_relation_nn; reference relation_network nn.py:115-190, geometric_encoding nn.py:273-298,
// from models.py:1044-1054): 16-head self-attention over the proposals of ONE image with a geometric bias on the logits.  Both
// products multiply activations by activations, so neither fits the conv kernels (their B operand is a weight image made at
// plan build).  Plain f32 in every arithmetic mode.  K proposal rows per image (blockIdx.z), of which the first n =
// min(count[b], K) are real; rows and columns >= n are zero or stale and are never read.
//   relation_geo_kernel        boxes [K,4] -> bias [16, K, Kp] (Kp = K rounded up to 4).  grid (ceil(K / 256), K): thread (i, j)
//             owns one pair: e = (log max(|dx| / w_i, 1e-3), log max(|dy| / w_i, 1e-3), log(w_i / w_j), log(h_i / h_j)) -- the y
//             term over w_i, as the reference has it --, g = tanh(e W_emb + b_emb) [64], a = g W_conv + b_conv [16], bias =
//             log(max(relu(a), 1e-6)).  The 1360 weights sit in LDS and are read as broadcasts; a[16] stays in registers.  Pairs
//             with i >= n or j >= n are not evaluated and their entries not written
//   relation_attention_kernel  grid (ceil(K / 16), 16 heads): a workgroup of 4 waves takes 16 query rows of one head.
//     scores   S[16, n] = Q_h K_h^T with v_mfma_f32_16x16x4_f32 over dh = D / 16 (operands straight from global: a fragment is
//              read once), times 1 / sqrt(dh), plus the bias, into LDS: one score row of up to 1024 columns per query (64 KB)
//     softmax  exact and two-pass in LDS, 16 threads per row: maximum, then exp and sum, each thread over its columns in index
//              order and the 16 partials by xor butterflies -- a fixed order, no atomics; P = e / sum overwrites S
//     output   O[16, D] = P v with the same MFMA, a wave per 64-column chunk of v (streamed from L2, which holds the [n, D]
//              tensor), P fragments from LDS; rows >= n are stored as zeros, rows >= K not at all.  The |max| of what is stored
//              goes to the range slot (publish_amax_wg), so that output_linear stays on the fp16x2 kernels
#include "conv_split_epilogue.hpp"

namespace odt {
namespace {

constexpr int kRelThreads = 256;
constexpr int kRelTile = 16;                      // query rows of a workgroup: one MFMA tile
constexpr int kRelPitch = kRelMaxK + 4;           // floats per score row in LDS (+4: the 16 rows of an A fragment fall into distinct banks)

__device__ __forceinline__ int rel_count(const int* count, int b, int K) {
  const int n = count[b];
  return n < 0 ? 0 : (n > K ? K : n);
}

__global__ void __launch_bounds__(kRelThreads) relation_geo_kernel(RelationGeoParams p) {
  __shared__ float w[kRelGeoWeights];
  const int tid = threadIdx.x;
  for (int t = tid; t < kRelGeoWeights; t += kRelThreads) w[t] = p.wts[t];
  __syncthreads();
  const int b = blockIdx.z, i = blockIdx.y, j = (int)blockIdx.x * kRelThreads + tid;
  const int n = rel_count(p.count, b, p.K);
  if (i >= n || j >= n) return;
  const float* we = w;                                        // geo_emb/W [4][64]
  const float* be = w + 4 * kRelGeoDim;                       // geo_emb/b [64]
  const float* wc = be + kRelGeoDim;                          // geo_conv/W [64][16]
  const float* bc = wc + kRelGeoDim * kRelHeads;              // geo_conv/b [16]
  const float* bi = p.boxes + ((size_t)b * p.K + i) * 4;
  const float* bj = p.boxes + ((size_t)b * p.K + j) * 4;
  const float wi = bi[2] - bi[0], hi = bi[3] - bi[1], cxi = 0.5f * (bi[0] + bi[2]), cyi = 0.5f * (bi[1] + bi[3]);
  const float wj = bj[2] - bj[0], hj = bj[3] - bj[1], cxj = 0.5f * (bj[0] + bj[2]), cyj = 0.5f * (bj[1] + bj[3]);
  const float e0 = logf(fmaxf(fabsf((cxi - cxj) / wi), 1e-3f));
  const float e1 = logf(fmaxf(fabsf((cyi - cyj) / wi), 1e-3f));
  const float e2 = logf(wi / wj);
  const float e3 = logf(hi / hj);
  float a[kRelHeads];
#pragma unroll
  for (int h = 0; h < kRelHeads; ++h) a[h] = bc[h];
  for (int k = 0; k < kRelGeoDim; ++k) {
    float s = e0 * we[k];
    s = fmaf(e1, we[kRelGeoDim + k], s);
    s = fmaf(e2, we[2 * kRelGeoDim + k], s);
    s = fmaf(e3, we[3 * kRelGeoDim + k], s);
    const float g = tanhf(s + be[k]);
#pragma unroll
    for (int h = 0; h < kRelHeads; ++h) a[h] = fmaf(g, wc[k * kRelHeads + h], a[h]);
  }
  float* o = p.bias + (((size_t)b * kRelHeads) * p.K + i) * p.Kp + j;
  const size_t hs = (size_t)p.K * p.Kp;
#pragma unroll
  for (int h = 0; h < kRelHeads; ++h) o[h * hs] = logf(fmaxf(fmaxf(a[h], 0.f), 1e-6f));
}

__global__ void __launch_bounds__(kRelThreads) relation_attention_kernel(RelationAttnParams p) {
  __shared__ __attribute__((aligned(16))) float S[kRelTile][kRelPitch];
  __shared__ __attribute__((aligned(16))) float red[kRelThreads / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.z, h = blockIdx.y, i0 = (int)blockIdx.x * kRelTile;
  const int K = p.K, D = p.D, dh = D / kRelHeads;
  const int n = rel_count(p.count, b, K);
  float* out = p.out + (size_t)b * K * kRelHeads * D;
  if (i0 >= n) {
    // a tile of padded rows (and every tile where n = 0): zeros, so that the GEMM behind reads finite data
    const int rows = K - i0 < kRelTile ? K - i0 : kRelTile, q4 = D >> 2;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    for (int t = tid; t < rows * q4; t += kRelThreads) {
      const int r = t / q4, c = t - r * q4;
      *reinterpret_cast<f32x4*>(out + ((size_t)(i0 + r) * kRelHeads + h) * D + c * 4) = zero;
    }
    return;
  }
  const int fr = lane & 15, fk = lane >> 4;      // MFMA 16x16x4: A[i = fr][k = fk], B[k = fk][j = fr], C rows 4 fk + r, column fr
  // ---- scores
  {
    const float scale = 1.0f / sqrtf((float)dh);
    const float* qrow = p.q + ((size_t)b * K + i0 + fr) * p.qk_ldc + h * dh + fk;
    const bool qok = i0 + fr < n;
    const float* bias = p.bias + (((size_t)b * kRelHeads + h) * K + i0) * p.Kp;
    const int ntile = (n + 15) >> 4;
    for (int jt = wave; jt < ntile; jt += kRelThreads / 64) {
      const int j = jt * 16 + fr;
      const bool kok = j < n;
      const float* krow = p.k + ((size_t)b * K + j) * p.qk_ldc + h * dh + fk;
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      for (int k0 = 0; k0 < dh; k0 += 4) {
        const float av = qok ? qrow[k0] : 0.f;
        const float bv = kok ? krow[k0] : 0.f;
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc, 0, 0, 0);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = 4 * fk + r;
        if (kok && i0 + row < n) S[row][j] = acc[r] * scale + bias[(size_t)row * p.Kp + j];
      }
    }
  }
  __syncthreads();
  // ---- softmax over j < n; a row >= n becomes zeros.  Columns n .. n4 - 1 (the k-step of the product below) are zeros too
  const int n4 = (n + 3) & ~3;
  {
    const int row = tid >> 4, t = tid & 15;
    float* s = S[row];
    const int nn = i0 + row < n ? n : 0;         // (every lane takes the shuffles)
    float mx = -INFINITY;
    for (int j = t; j < nn; j += 16) mx = fmaxf(mx, s[j]);
#pragma unroll
    for (int d = 8; d >= 1; d >>= 1) mx = fmaxf(mx, __shfl_xor(mx, d));
    float sum = 0.f;
    for (int j = t; j < nn; j += 16) {
      const float e = expf(s[j] - mx);
      s[j] = e;
      sum += e;
    }
#pragma unroll
    for (int d = 8; d >= 1; d >>= 1) sum += __shfl_xor(sum, d);
    for (int j = t; j < nn; j += 16) s[j] = s[j] / sum;
    for (int j = nn + t; j < n4; j += 16) s[j] = 0.f;
  }
  __syncthreads();
  // ---- output
  float vmax = 0.f;
  for (int cc = wave; cc < (D >> 6); cc += kRelThreads / 64) {
    const int c0 = cc * 64 + fr;
    f32x4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < n4; k0 += 4) {
      const int kk = k0 + fk;
      const float av = S[fr][kk];
      const bool ok = kk < n;
      const float* vr = p.v + ((size_t)b * K + kk) * p.v_ldc + c0;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const float bv = ok ? vr[16 * t] : 0.f;
        acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc[t], 0, 0, 0);
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = i0 + 4 * fk + r;
      if (i >= K) continue;
      float* o = out + ((size_t)i * kRelHeads + h) * D + c0;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const float y = i < n ? acc[t][r] : 0.f;
        o[16 * t] = y;
        vmax = fmaxf(vmax, fabsf(y));
      }
    }
  }
  publish_amax_wg<kRelThreads>(p.amax, vmax, tid, reinterpret_cast<unsigned char*>(red));
}

}  // namespace

int launch_relation_geo(const RelationGeoParams& p, hipStream_t stream) {
  ODT_CHECK(p.boxes && p.count && p.wts && p.bias, "relation_geo: null argument");
  ODT_CHECK(p.B >= 1 && p.B <= 65535 && p.K >= 1, "relation_geo: bad sizes");
  ODT_CHECK(p.K <= kRelMaxK, "relation_geo: at most " + std::to_string(kRelMaxK) + " proposals per image (K = " + std::to_string(p.K) + ")");
  ODT_CHECK(p.Kp == relation_kp(p.K), "relation_geo: the bias rows must be K rounded up to 4 floats");
  hipLaunchKernelGGL(relation_geo_kernel, dim3((unsigned)((p.K + kRelThreads - 1) / kRelThreads), (unsigned)p.K, (unsigned)p.B),
                     dim3(kRelThreads), 0, stream, p);
  ODT_HIP(hipGetLastError());
  return 0;
}

int launch_relation_attention(const RelationAttnParams& p, hipStream_t stream) {
  ODT_CHECK(p.q && p.k && p.v && p.bias && p.count && p.out, "relation_attention: null argument");
  ODT_CHECK(p.B >= 1 && p.B <= 65535 && p.K >= 1, "relation_attention: bad sizes");
  ODT_CHECK(p.K <= kRelMaxK, "relation_attention: at most " + std::to_string(kRelMaxK) + " proposals per image (K = " + std::to_string(p.K) +
                                 "): a query keeps one score row in LDS");
  ODT_CHECK(p.D >= 64 && p.D <= kRelMaxD && p.D % 64 == 0,
            "relation_attention: D must be a multiple of 64 in [64, " + std::to_string(kRelMaxD) + "] (D = " + std::to_string(p.D) + ")");
  ODT_CHECK(p.Kp == relation_kp(p.K), "relation_attention: the bias rows must be K rounded up to 4 floats");
  ODT_CHECK(p.qk_ldc >= p.D && p.v_ldc >= p.D, "relation_attention: a row pitch is smaller than D");
  ODT_CHECK(((uintptr_t)p.out & 15) == 0, "relation_attention: out must be 16-byte aligned");
  hipLaunchKernelGGL(relation_attention_kernel, dim3((unsigned)((p.K + kRelTile - 1) / kRelTile), (unsigned)kRelHeads, (unsigned)p.B),
                     dim3(kRelThreads), 0, stream, p);
  ODT_HIP(hipGetLastError());
  return 0;
}

}  // namespace odt
