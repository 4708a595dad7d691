// Mask paste + COCO run-length encoding of the Mask R-CNN output (reference obj_detect_tracking.py:715-739,
// obj_detect_imgs.py:504-527: final_boxes / scale -> fill_full_mask(box, mask, im.shape[:2]), nn.py:1565-1584 ->
// pycocotools mask.encode of the column-major frame -> counts.decode("ascii")).
//
// Per detection j: b = final_boxes[j] / scale (f32), x0 = int(b0 + 0.5f), y0 = int(b1 + 0.5f), x1 = max(x0, int(b2 - 0.5f)),
// y1 = max(y0, int(b3 - 0.5f)); the 28x28 mask resized to (y1 + 1 - y0) x (x1 + 1 - x0) with the INTER_LINEAR rule of the ingest
// resize (elementwise.hip preprocess_resize_kernel: taps in double, weights in f32, the horizontal blend first), thresholded
// with > 0.5 and pasted at [y0:y1+1, x0:x1+1] of an all-zero H0 x W0 frame.  The frame is never materialised: a run boundary
// ("transition") is a column-major index x * H0 + y whose pixel differs from the one before it, and the counts are the
// differences of 0, the transitions in order, H0 * W0.  Where the reference would raise (a rectangle past the frame) the
// rectangle is clipped to the frame.
//
// mask_rle_runs_kernel: one workgroup per detection walks the clipped rectangle's columns in chunks of 256.  A wave
// evaluates 64 rows of one column per step and takes them as one __ballot word; its transitions are
// bits ^ (bits << 1 | carry).  Pass 1 counts them per column, a workgroup scan turns the counts into offsets, pass 2
// evaluates the same columns again and writes the transitions in order.  At most kRleTransPerCol * W0 + 1 transitions per
// detection (27 source intervals per column plus the entry and the exit: 29 in exact arithmetic); a detection past that
// bound writes nothing more and reports -1 (the entry points fail the call and name it).  Then the workgroup sums the
// length of its compressed string.
// mask_rle_strings_kernel: one workgroup per detection packs its string (and, optionally, its counts) behind those of the
// detections before it: the offset is the sum of their lengths, a workgroup scan places the characters of each count.
// Integer arithmetic only after the threshold: the output does not depend on scheduling.
#include <cmath>
#include <functional>

#include "odt_common.hpp"

namespace odt {

namespace {

constexpr int kRleThreads = 256;      // 4 waves
constexpr int kRleCols = 256;         // columns per chunk of the runs kernel

// pycocotools rleToString: 5-bit groups, low first, continuation bit 0x20, offset 48
__device__ __forceinline__ int rle_chars(long long x) {
  int n = 0;
  bool more;
  do {
    const int c = (int)(x & 0x1f);
    x >>= 5;
    more = (c & 0x10) ? x != -1 : x != 0;
    ++n;
  } while (more);
  return n;
}

__device__ __forceinline__ void rle_put(char* o, long long x) {
  int n = 0;
  bool more;
  do {
    int c = (int)(x & 0x1f);
    x >>= 5;
    more = (c & 0x10) ? x != -1 : x != 0;
    if (more) c |= 0x20;
    o[n++] = (char)(c + 48);
  } while (more);
}

// count i (0..n) of a detection with n transitions t[]: t[i] - t[i - 1], with t[-1] = 0 and t[n] = H0 * W0
__device__ __forceinline__ long long rle_count(const int* t, int n, int i, long long area) {
  const long long hi = i < n ? (long long)t[i] : area;
  const long long lo = i > 0 ? (long long)t[i - 1] : 0;
  return hi - lo;
}

// the value rleToString encodes for count i (cnts[i] - cnts[i - 2] for i > 2)
__device__ __forceinline__ long long rle_delta(const int* t, int n, int i, long long area) {
  const long long c = rle_count(t, n, i, area);
  return i > 2 ? c - rle_count(t, n, i - 2, area) : c;
}

__device__ __forceinline__ long long block_sum(long long v, long long* red) {
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  const long long s = red[0] + red[1] + red[2] + red[3];
  __syncthreads();
  return s;
}

// exclusive scan of one int per thread over the 256-thread workgroup; *total = the sum
__device__ __forceinline__ int block_excl_scan(int v, int* wsum, int* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int s = v;
  for (int d = 1; d < 64; d <<= 1) {
    const int t = __shfl_up(s, d);
    if (lane >= d) s += t;
  }
  if (lane == 63) wsum[wave] = s;
  __syncthreads();
  int below = 0, tot = 0;
  for (int k = 0; k < kRleThreads / 64; ++k) {
    if (k < wave) below += wsum[k];
    tot += wsum[k];
  }
  __syncthreads();
  *total = tot;
  return below + s - v;
}

// the box of a detection in frame pixels (fill_full_mask's integer rectangle) and its part inside the frame
struct RleBox { int x0, y0, w, h, cx0, cx1, cy0, cy1; };

__device__ __forceinline__ int trunc_coord(float v) {
  // int() truncates toward zero; boxes of any realistic size pass unchanged (the clamp keeps the conversion defined)
  v = v != v ? 0.f : (v < -268435456.f ? -268435456.f : (v > 268435456.f ? 268435456.f : v));
  return (int)v;
}

__device__ __forceinline__ RleBox rle_box(const MaskRleParams& p, int j) {
  const float* b = p.boxes + (size_t)j * 4;
  const float bx0 = b[0] / p.scale, by0 = b[1] / p.scale, bx1 = b[2] / p.scale, by1 = b[3] / p.scale;
  RleBox r;
  r.x0 = trunc_coord(bx0 + 0.5f);
  r.y0 = trunc_coord(by0 + 0.5f);
  int x1 = trunc_coord(bx1 - 0.5f), y1 = trunc_coord(by1 - 0.5f);
  x1 = x1 > r.x0 ? x1 : r.x0;
  y1 = y1 > r.y0 ? y1 : r.y0;
  r.w = x1 + 1 - r.x0;
  r.h = y1 + 1 - r.y0;
  r.cx0 = r.x0 > 0 ? r.x0 : 0;
  r.cy0 = r.y0 > 0 ? r.y0 : 0;
  r.cx1 = x1 < p.W0 - 1 ? x1 : p.W0 - 1;
  r.cy1 = y1 < p.H0 - 1 ? y1 : p.H0 - 1;
  return r;
}

// INTER_LINEAR taps of destination index d of an n_dst-long axis over the 28 source samples (nn._axis_taps)
__device__ __forceinline__ void rle_tap(int d, int n_dst, int* i0, int* i1, float* w1) {
  const double f = ((double)d + 0.5) * (28.0 / (double)n_dst) - 0.5;
  int a = (int)floor(f);
  double fr = f - (double)a;
  if (a < 0) { a = 0; fr = 0.0; }
  if (a >= 27) { a = 27; fr = 0.0; }
  *i0 = a;
  *i1 = a + 1 < 28 ? a + 1 : 27;
  *w1 = (float)fr;
}

// one frame pixel of the pasted mask from the mask in LDS: the operations and order of the column walk below
__device__ __forceinline__ bool rle_pixel(const float* msk, const RleBox& r, int x, int ytap, float wy) {
  int xs0, xs1;
  float wx;
  rle_tap(x - r.x0, r.w, &xs0, &xs1, &wx);
  const float omx = 1.0f - wx;
  const int ys0 = ytap & 0xff, ys1 = ytap >> 8;
  const float top = msk[ys0 * 28 + xs0] * omx + msk[ys0 * 28 + xs1] * wx;
  const float bot = msk[ys1 * 28 + xs0] * omx + msk[ys1 * 28 + xs1] * wx;
  return top * (1.0f - wy) + bot * wy > 0.5f;
}

// column x of the clipped rectangle, by one whole wave: the number of transitions the column owns, written to out[0..)
// when out != nullptr.  The column owns the positions of its rows cy0..cy1 (each compared with the pixel before it in
// column-major order) and the position after its last row when the next column does not own that one.
__device__ int rle_column(const MaskRleParams& p, const float* msk, const int* rtap, const float* rw, const RleBox& r, int x,
                          int* out) {
  const int lane = threadIdx.x & 63;
  int xs0, xs1;
  float wx;
  rle_tap(x - r.x0, r.w, &xs0, &xs1, &wx);
  const float omx = 1.0f - wx;
  // the horizontal pass: lane l < 28 holds source row l blended at this column
  const float hv = lane < 28 ? msk[lane * 28 + xs0] * omx + msk[lane * 28 + xs1] * wx : 0.f;
  const bool full_h = r.cy0 == 0 && r.cy1 == p.H0 - 1;
  // the pixel before row 0 is the last row of the previous column: inside the rectangle only for a full-height one
  unsigned long long carry = 0;
  if (full_h && x > r.cx0) {
    const int last = r.cy1 - r.cy0;
    carry = rle_pixel(msk, r, x - 1, rtap[last], rw[last]) ? 1ull : 0ull;
  }
  const long long col = (long long)x * p.H0;
  int cnt = 0, last_bit = 0;
  for (int y0 = r.cy0; y0 <= r.cy1; y0 += 64) {
    const int y = y0 + lane;
    const bool in = y <= r.cy1;
    const int t = in ? rtap[y - r.cy0] : 0;
    const float wy = in ? rw[y - r.cy0] : 0.f;
    const float top = __shfl(hv, t & 0xff), bot = __shfl(hv, t >> 8);
    const bool bit = in && top * (1.0f - wy) + bot * wy > 0.5f;
    const unsigned long long bits = __ballot(bit);
    const int nin = r.cy1 - y0 + 1 < 64 ? r.cy1 - y0 + 1 : 64;
    const unsigned long long inmask = nin == 64 ? ~0ull : ((1ull << nin) - 1ull);
    const unsigned long long tr = (bits ^ ((bits << 1) | carry)) & inmask;
    if (out != nullptr && ((tr >> lane) & 1ull))
      out[cnt + __popcll(tr & ((1ull << lane) - 1ull))] = (int)(col + y);
    cnt += __popcll(tr);
    carry = bits >> 63;
    last_bit = (int)((bits >> (nin - 1)) & 1ull);
  }
  // the exit after the last row: owned by the next column (full-height rectangle), or the end of the frame
  const bool owned_next = r.cy1 == p.H0 - 1 && ((r.cy0 == 0 && x < r.cx1) || x == p.W0 - 1);
  if (last_bit && !owned_next) {
    if (out != nullptr && lane == 0) out[cnt] = (int)(col + r.cy1 + 1);
    ++cnt;
  }
  return cnt;
}

__global__ void __launch_bounds__(kRleThreads) mask_rle_runs_kernel(MaskRleParams p) {
  __shared__ float msk[784];
  __shared__ int rtap[kRleMaxH];      // per clipped row: source rows ys0 | ys1 << 8
  __shared__ float rw[kRleMaxH];      // ... and the weight of ys1
  __shared__ int colv[kRleCols];      // per column of the chunk: its transitions, then their offset
  __shared__ int wsum[kRleThreads / 64];
  __shared__ long long red[kRleThreads / 64];
  const int j = blockIdx.x, tid = threadIdx.x, wave = tid >> 6;
  const int nvalid = p.valid != nullptr ? *p.valid : p.n;
  if (j >= nvalid) {
    if (tid == 0) { p.ntrans[j] = 0; p.slen[j] = 0; }
    return;
  }
  const RleBox r = rle_box(p, j);
  for (int i = tid; i < 784; i += kRleThreads) msk[i] = p.masks[(size_t)j * 784 + i];
  const int nrow = r.cy1 - r.cy0 + 1;
  for (int i = tid; i < nrow; i += kRleThreads) {
    int a, b;
    float w1;
    rle_tap(r.cy0 + i - r.y0, r.h, &a, &b, &w1);
    rtap[i] = a | (b << 8);
    rw[i] = w1;
  }
  __syncthreads();
  int* out = p.trans + (size_t)j * p.cap;
  int base = 0;
  bool overflow = false;
  for (int c0 = r.cx0; c0 <= r.cx1 && nrow > 0; c0 += kRleCols) {
    const int ncol = r.cx1 - c0 + 1 < kRleCols ? r.cx1 - c0 + 1 : kRleCols;
    for (int c = wave; c < ncol; c += kRleThreads / 64) {
      const int n = rle_column(p, msk, rtap, rw, r, c0 + c, nullptr);
      if ((tid & 63) == 0) colv[c] = n;
    }
    __syncthreads();
    const int mine = tid < ncol ? colv[tid] : 0;
    int total;
    const int off = block_excl_scan(mine, wsum, &total);
    if (tid < ncol) colv[tid] = off;
    __syncthreads();
    if (total > p.cap - base) { overflow = true; break; }     // (the same for every thread)
    for (int c = wave; c < ncol; c += kRleThreads / 64) rle_column(p, msk, rtap, rw, r, c0 + c, out + base + colv[c]);
    base += total;
    __syncthreads();
  }
  if (overflow) {
    if (tid == 0) { p.ntrans[j] = -1; p.slen[j] = 0; }
    return;
  }
  __syncthreads();      // the transitions this workgroup wrote are visible to all of its threads
  const long long area = (long long)p.H0 * p.W0;
  long long len = 0;
  for (int i = tid; i <= base; i += kRleThreads) len += rle_chars(rle_delta(out, base, i, area));
  len = block_sum(len, red);
  if (tid == 0) { p.ntrans[j] = base; p.slen[j] = (int)len; }
}

__global__ void __launch_bounds__(kRleThreads) mask_rle_strings_kernel(MaskRleParams p) {
  __shared__ int wsum[kRleThreads / 64];
  __shared__ long long red[kRleThreads / 64];
  const int j = blockIdx.x, tid = threadIdx.x;
  const int nvalid = p.valid != nullptr ? *p.valid : p.n;
  if (j >= nvalid) return;
  long long so = 0, co = 0;
  for (int i = tid; i < j; i += kRleThreads) { so += p.slen[i]; co += p.ntrans[i] + 1; }
  so = block_sum(so, red);
  co = block_sum(co, red);
  const int n = p.ntrans[j];
  const int* t = p.trans + (size_t)j * p.cap;
  const long long area = (long long)p.H0 * p.W0;
  char* s = p.str + so;
  for (int i0 = 0; i0 <= n; i0 += kRleThreads) {
    const int i = i0 + tid;
    const long long x = i <= n ? rle_delta(t, n, i, area) : 0;
    int total;
    const int pos = block_excl_scan(i <= n ? rle_chars(x) : 0, wsum, &total);
    if (i <= n) {
      rle_put(s + pos, x);
      if (p.counts != nullptr) p.counts[co + i] = (unsigned)rle_count(t, n, i, area);
    }
    s += total;
  }
}

}  // namespace

int launch_mask_rle_runs(const MaskRleParams& p, hipStream_t stream) {
  ODT_CHECK(p.R >= 1 && p.H0 >= 1 && p.W0 >= 1 && p.H0 <= kRleMaxH, "mask_rle: bad sizes");
  hipLaunchKernelGGL(mask_rle_runs_kernel, dim3(p.R), dim3(kRleThreads), 0, stream, p);
  ODT_HIP(hipGetLastError());
  return 0;
}

int launch_mask_rle_strings(const MaskRleParams& p, hipStream_t stream) {
  hipLaunchKernelGGL(mask_rle_strings_kernel, dim3(p.R), dim3(kRleThreads), 0, stream, p);
  ODT_HIP(hipGetLastError());
  return 0;
}

int run_mask_rle(MaskRleParams p, bool want_counts, hipStream_t st, const RleAlloc& alloc, MaskRleHost& out) {
  ODT_CHECK(p.H0 >= 1 && p.W0 >= 1, "mask_rle: the frame size must be positive");
  ODT_CHECK(p.H0 <= kRleMaxH, "mask_rle: frames taller than " + std::to_string(kRleMaxH) + " rows are not supported");
  ODT_CHECK((long long)p.H0 * p.W0 < (1ll << 31), "mask_rle: frames of 2^31 pixels or more are not supported");
  ODT_CHECK(p.scale > 0.f && std::isfinite(p.scale), "mask_rle: scale must be a positive number");
  out.n = 0; out.H0 = p.H0; out.W0 = p.W0;
  out.str.clear(); out.off.clear(); out.len.clear(); out.counts.clear(); out.coff.assign(1, 0);
  if (p.R == 0) return 0;
  p.cap = kRleTransPerCol * p.W0 + 1;
  int* meta = nullptr;      // [ntrans | slen]
  if (alloc("transitions", (size_t)p.R * p.cap * sizeof(int), (void**)&p.trans) ||
      alloc("sizes", 2 * (size_t)p.R * sizeof(int), (void**)&meta)) return 1;
  p.ntrans = meta; p.slen = meta + p.R;
  p.str = nullptr; p.counts = nullptr;
  if (launch_mask_rle_runs(p, st)) return 1;
  std::vector<int> h(2 * (size_t)p.R + 1);
  ODT_HIP(hipMemcpyAsync(h.data(), meta, 2 * (size_t)p.R * sizeof(int), hipMemcpyDeviceToHost, st));
  if (p.valid != nullptr) ODT_HIP(hipMemcpyAsync(h.data() + 2 * (size_t)p.R, p.valid, sizeof(int), hipMemcpyDeviceToHost, st));
  ODT_HIP(hipStreamSynchronize(st));
  const int n = p.valid != nullptr ? h[2 * (size_t)p.R] : p.n;
  ODT_CHECK(n >= 0 && n <= p.R, "mask_rle: bad number of detections");
  size_t bytes = 0, ncounts = 0;
  out.off.resize(n); out.len.resize(n); out.coff.resize((size_t)n + 1);
  for (int j = 0; j < n; ++j) {
    ODT_CHECK(h[j] >= 0, "mask_rle: detection " + std::to_string(j) + " has more than " + std::to_string(p.cap) +
                             " run boundaries (the bound of " + std::to_string(kRleTransPerCol) + " per frame column)");
    out.off[j] = (int64_t)bytes; out.len[j] = h[p.R + j];
    bytes += (size_t)h[p.R + j];
    out.coff[j] = (int64_t)ncounts;
    ncounts += (size_t)h[j] + 1;
  }
  out.coff[n] = (int64_t)ncounts;
  out.n = n;
  if (n == 0) return 0;
  if (alloc("strings", bytes, (void**)&p.str)) return 1;
  if (want_counts && alloc("counts", ncounts * sizeof(unsigned), (void**)&p.counts)) return 1;
  if (launch_mask_rle_strings(p, st)) return 1;
  out.str.resize(bytes);
  ODT_HIP(hipMemcpyAsync(out.str.data(), p.str, bytes, hipMemcpyDeviceToHost, st));
  if (want_counts) {
    out.counts.resize(ncounts);
    ODT_HIP(hipMemcpyAsync(out.counts.data(), p.counts, ncounts * sizeof(unsigned), hipMemcpyDeviceToHost, st));
  }
  ODT_HIP(hipStreamSynchronize(st));
  return 0;
}

}  // namespace odt
