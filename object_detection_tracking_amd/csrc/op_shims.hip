// Stand-alone op entry points of the C ABI (include/odt.h: odt_op_*, odt_nn_cosine): host pointers in and out, each
// runs exactly the kernels the forward uses -- what the staged parity tests call.  The fusion shims (odt_op_bottleneck_tail,
// odt_op_bottleneck_block, odt_op_stem) turn their records into the fused ones with the functions the plan's fuse_* passes call
// (conv_h2f_fuse, conv_block_fuse, conv_stem_fuse: odt_common.hpp), so a test of a shim tests the plan's rewrite.
#include <functional>

#include "odt_model.hpp"

using namespace odt;
#define g_err (::odt::last_error())

namespace {

template <typename T>
struct Tmp {   // RAII device temp for the stand-alone ops
  T* d = nullptr;
  size_t n = 0;
  int alloc(size_t count) { n = count; ODT_HIP(hipMalloc((void**)&d, (count ? count : 1) * sizeof(T))); return 0; }
  int put(const T* h) { ODT_HIP(hipMemcpy(d, h, n * sizeof(T), hipMemcpyHostToDevice)); return 0; }
  int get(T* h, size_t count) { ODT_HIP(hipMemcpy(h, d, count * sizeof(T), hipMemcpyDeviceToHost)); return 0; }
  int zero() { ODT_HIP(hipMemset(d, 0, (n ? n : 1) * sizeof(T))); return 0; }
  ~Tmp() { if (d) (void)hipFree(d); }
};

int set_dev(int device) {
  int n = 0;
  ODT_HIP(hipGetDeviceCount(&n));
  ODT_CHECK(device >= 0 && device < n, "no such device");
  ODT_HIP(hipSetDevice(device));
  return 0;
}

// what the stand-alone conv entry points launched last on this thread (odt_op_last_conv): the finished record's row and
// launch choices, kept at the launch points below.  Host only; nothing on the plan's path writes or reads it.
struct LastConv { int variant = CV_NONE, splitk = 0, reduce_blocks = 0; };
thread_local LastConv g_last_conv;
void note_conv(const ConvParams& q) { g_last_conv.variant = q.variant; g_last_conv.splitk = q.splitk; g_last_conv.reduce_blocks = q.reduce_blocks; }

// the ODT_CONV_CHOICE_OUT fields and the row name of a finished record (odt_op_conv_choice, odt_op_last_conv)
void conv_report(int variant, int splitk, int reduce_blocks, int* out, char* name, int name_cap) {
  const ConvKernelRow& r = conv_variant_row(variant);
  for (int i = 0; i < ODT_CONV_CHOICE_OUT; ++i) out[i] = 0;
  if (name && name_cap > 0) { std::strncpy(name, r.name, name_cap - 1); name[name_cap - 1] = 0; }
  if (r.family != CF_F32) {
    out[0] = 1; out[1] = r.family; out[2] = r.bm; out[3] = r.bn; out[4] = (r.flags & CVF_KWR) ? 1 : 0; out[5] = splitk;
    out[6] = (r.flags & CVF_DSTAGE) ? 1 : 0; out[10] = reduce_blocks;
  } else {
    out[7] = r.bn == 128 ? 3 : (r.bm == 64 ? 2 : 1); out[8] = (r.flags & CVF_ST2) ? 2 : 1; out[9] = (r.flags & CVF_FINE) ? 1 : 0;
  }
}

// a conv record over dense tensors: in [B,H,W,Cin] -> out [B,Ho,Wo,Cout], wt [Cout][kh][kw][Cin].  Residual, output offset and
// second source: the callers that have one set them.
ConvParams dense_conv(const float* in, const float* wt, const float* bias, float* out, int B, int H, int W, int Cin, int Ho, int Wo,
                      int Cout, int kh, int kw, int stride, int dil, int pad_t, int pad_l, int relu) {
  ConvParams p; std::memset(&p, 0, sizeof(p));
  p.in = in; p.wt = wt; p.bias = bias; p.out = out;
  p.B = B; p.H = H; p.W = W; p.Cin = Cin; p.in_ldc = Cin; p.in_Ha = H; p.in_Wa = W; p.Ho = Ho; p.Wo = Wo; p.Cout = Cout;
  p.kh = kh; p.kw = kw; p.stride = stride; p.dil = dil; p.pad_t = pad_t; p.pad_l = pad_l;
  p.out_H = Ho; p.out_W = Wo; p.out_ldc = Cout; p.relu = relu;
  return p;
}
// ... the bottleneck's convs: k x k, stride 1, 'SAME' for dilation dil, same size out
ConvParams same_conv(const float* in, const float* wt, const float* bias, float* out, int B, int H, int W, int Cin, int Cout, int k,
                     int dil, int relu) {
  return dense_conv(in, wt, bias, out, B, H, W, Cin, H, W, Cout, k, k, 1, dil, dil * (k - 1) / 2, dil * (k - 1) / 2, relu);
}

// HWIO weights [kh][kw][Cin][Cout] in the kernels' order [Cout][kh][kw][Cin] (a 1x1 conv's "IO" matrix: kh = kw = 1)
std::vector<float> ohwi(const float* hwio, int kh, int kw, int Cin, int Cout) {
  std::vector<float> w((size_t)Cout * kh * kw * Cin);
  for (int t = 0; t < kh * kw; ++t) for (int i = 0; i < Cin; ++i) for (int o = 0; o < Cout; ++o)
    w[((size_t)o * kh * kw + t) * Cin + i] = hwio[((size_t)t * Cin + i) * Cout + o];
  return w;
}

// this record runs row `variant` on the fp16x2 kernels: its sources' and its output's range slots, the derived fields, its
// weight image in img
int use_h2_row(ConvParams& p, int variant, const unsigned* in_amax, unsigned* out_amax, Tmp<float>& img) {
  conv_use_variant(p, variant);
  p.in_amax = in_amax; p.out_amax = out_amax;
  conv_prepare(p);
  if (img.alloc((conv_split_weight_bytes(p.Cout, conv_k(p)) + 3) / 4) || conv_make_split_weights(p, img.d, nullptr)) return 1;
  conv_attach_weights(p, img.d);
  return 0;
}

// one stand-alone conv (odt_op_conv2d*: dense tensors, null stream) as a plan would run it: the library's policy under the
// call's knobs, a temporary weight image / split-K scratch / input range where the split kernels take it, a finished record
int run_conv(ConvParams q, const Knobs& kn) {
  if (conv_check(q)) return 1;
  conv_prepare(q);
  struct Temps {                      // released on every path out of this function
    void* img = nullptr; float* partial = nullptr; unsigned* amax = nullptr; ConvParams* rec = nullptr;
    ~Temps() {
      (void)hipStreamSynchronize(nullptr);
      if (rec) (void)hipFree(rec);
      if (img) (void)hipFree(img);
      if (partial) (void)hipFree(partial);
      if (amax) (void)hipFree(amax);
    }
  } tmp;
  const ConvPolicy pol = conv_policy_with_knobs(conv_policy_default(), kn);
  ConvChoice ch = conv_select(q, pol, kn);
  if (conv_variant_row(ch.variant).family != CF_F32) {
    ODT_HIP(hipMalloc(&tmp.img, conv_split_weight_bytes(q.Cout, conv_k(q))));
    if (pol.family == 2 && q.in_amax == nullptr) {      // fp16x2 pieces need the sources' |max|: nobody recorded it for a stand-alone call
      // (the scan covers the whole allocation B x in_Ha x in_Wa x in_ldc of a source: a stand-alone caller hands over
      // dense tensors -- odt_op_conv2d* -- so this is the logical view; a sliced view would have to bring its own range)
      ODT_HIP(hipMalloc((void**)&tmp.amax, 2 * kAmaxWays * sizeof(unsigned)));
      ODT_HIP(hipMemsetAsync(tmp.amax, 0, 2 * kAmaxWays * sizeof(unsigned), nullptr));
      if (launch_tensor_amax(q.in, (size_t)q.B * q.in_Ha * q.in_Wa * q.in_ldc, tmp.amax, nullptr)) return 1;
      q.in_amax = tmp.amax;
      if (q.in2 != nullptr) {
        if (launch_tensor_amax(q.in2, (size_t)q.B * q.in2_Ha * q.in2_Wa * q.in2_ldc, tmp.amax + kAmaxWays, nullptr)) return 1;
        q.in2_amax = tmp.amax + kAmaxWays;
      }
      ch = conv_select(q, pol, kn);       // (with the ranges: whether a layer takes the split kernels does not depend on them, which ones does)
    }
    conv_use_variant(q, ch.variant, ch.splitk, ch.reduce_blocks);
    if (conv_make_split_weights(q, tmp.img, nullptr)) return 1;
    conv_attach_weights(q, tmp.img);
    if (conv_split_partial_bytes(q) > 0) ODT_HIP(hipMalloc((void**)&tmp.partial, conv_split_partial_bytes(q)));
    q.partial = tmp.partial;
  }
  if (conv_finish(q, kn)) return 1;
  note_conv(q);
  ODT_HIP(hipMalloc((void**)&tmp.rec, sizeof(ConvParams)));
  ODT_HIP(hipMemcpy(tmp.rec, &q, sizeof(ConvParams), hipMemcpyHostToDevice));
  return launch_conv(q, tmp.rec, nullptr);
}

// ODT_CONV_TRACE report of odt_op_conv2d (tuning aid): per-phase wall-clock (100 MHz) statistics over the workgroups
int report_conv_trace(Tmp<unsigned long long>& tr, int max_blocks) {
  std::vector<unsigned long long> t((size_t)max_blocks * 16);
  if (tr.get(t.data(), t.size())) return 1;
  unsigned long long t0 = ~0ull, t1 = 0; int nb = 0;
  double ph[5] = {0, 0, 0, 0, 0};
  for (int b = 0; b < max_blocks; ++b) {
    const unsigned long long* q = &t[(size_t)b * 16];
    if (q[0] == 0) continue;
    ++nb; if (q[0] < t0) t0 = q[0]; if (q[5] > t1) t1 = q[5];
    for (int i = 0; i < 5; ++i) ph[i] += (double)(q[i + 1] - q[i]);
  }
  printf("[conv trace] blocks=%d span=%.1f us | per block avg us: prologue %.2f  mainloop %.2f  res-issue+stage0 %.2f  "
         "pass0 lds->stores %.2f  pass1 %.2f | sum %.2f\n", nb, (t1 - t0) / 100.0, ph[0] / nb / 100, ph[1] / nb / 100,
         ph[2] / nb / 100, ph[3] / nb / 100, ph[4] / nb / 100, (ph[0] + ph[1] + ph[2] + ph[3] + ph[4]) / nb / 100);
  // concurrency: how many blocks are in the main loop at the midpoint of the launch
  const unsigned long long mid = t0 + (t1 - t0) / 2; int in_main = 0, in_epi = 0, in_pro = 0;
  for (int b = 0; b < max_blocks; ++b) {
    const unsigned long long* q = &t[(size_t)b * 16];
    if (q[0] == 0) continue;
    if (mid >= q[0] && mid < q[1]) ++in_pro; else if (mid >= q[1] && mid < q[2]) ++in_main; else if (mid >= q[2] && mid < q[5]) ++in_epi;
  }
  {   // first dispatch wave vs the rest
    double sa[3] = {0, 0, 0}, sb[3] = {0, 0, 0};
    double pa = 0, pb = 0, ma = 0, mb = 0; int na = 0, nb2 = 0;
    for (int b = 0; b < max_blocks; ++b) {
      const unsigned long long* q = &t[(size_t)b * 16];
      if (q[0] == 0) continue;
      double* sx = (q[0] - t0 < 500) ? sa : sb;
      sx[0] += (double)(q[6] - q[0]); sx[1] += (double)(q[7] - q[6]); sx[2] += (double)(q[1] - q[7]);
      if (q[0] - t0 < 500) { pa += (double)(q[1] - q[0]); ma += (double)(q[2] - q[1]); ++na; }
      else { pb += (double)(q[1] - q[0]); mb += (double)(q[2] - q[1]); ++nb2; }
    }
    printf("[conv trace] first wave (%d blocks): prologue %.2f us, mainloop %.2f us | later (%d blocks): prologue %.2f us, mainloop %.2f us\n",
           na, na ? pa / na / 100 : 0.0, na ? ma / na / 100 : 0.0, nb2, nb2 ? pb / nb2 / 100 : 0.0, nb2 ? mb / nb2 / 100 : 0.0);
    if (na && nb2)
      printf("[conv trace] prologue split (setup / first loads+lds / barrier): first wave %.2f / %.2f / %.2f us, later %.2f / %.2f / %.2f us\n",
             sa[0] / na / 100, sa[1] / na / 100, sa[2] / na / 100, sb[0] / nb2 / 100, sb[1] / nb2 / 100, sb[2] / nb2 / 100);
  }
  printf("[conv trace] at mid-launch: %d blocks in prologue, %d in main loop, %d in epilogue\n", in_pro, in_main, in_epi);
  {   // placement and per-CU concurrency: for every CU, the fraction of its busy time with 0 / 1 / 2 / 3+
      // resident workgroups inside the main loop (lockstep shows up as time with 0 in the loop)
    std::map<unsigned, std::vector<int>> cu_blocks;
    for (int b = 0; b < max_blocks; ++b) {
      const unsigned long long* q = &t[(size_t)b * 16];
      if (q[0] == 0) continue;
      const unsigned hw = (unsigned)q[8], xcc = (unsigned)q[9] & 0xf;
      const unsigned cu = (hw >> 8) & 0xf, sh = (hw >> 12) & 1, se = (hw >> 13) & 0x7;
      cu_blocks[(xcc << 12) | (se << 8) | (sh << 4) | cu].push_back(b);
    }
    double frac[4] = {0, 0, 0, 0}; double busy = 0;
    for (auto& kv : cu_blocks) {
      std::vector<std::pair<unsigned long long, int>> ev;   // (time, +1/-1) for main-loop occupancy
      unsigned long long lo = ~0ull, hi = 0;
      for (int b : kv.second) {
        const unsigned long long* q = &t[(size_t)b * 16];
        ev.push_back({q[1], +1}); ev.push_back({q[2], -1});
        if (q[0] < lo) lo = q[0]; if (q[5] > hi) hi = q[5];
      }
      std::sort(ev.begin(), ev.end());
      unsigned long long prev = lo; int n = 0;
      for (auto& e : ev) {
        frac[n > 3 ? 3 : n] += (double)(e.first - prev); prev = e.first; n += e.second;
      }
      frac[0] += (double)(hi - prev); busy += (double)(hi - lo);
    }
    printf("[conv trace] %zu CUs seen; time share per CU with k workgroups in the main loop: k=0 %.3f  k=1 %.3f  k=2 %.3f  k>=3 %.3f\n",
           cu_blocks.size(), frac[0] / busy, frac[1] / busy, frac[2] / busy, frac[3] / busy);
    // dispatch order on XCD 0: which CU did the first blocks land on
    printf("[conv trace] XCD0 first blocks -> (se,cu,tg): ");
    for (int b = 0; b < 8 * 40 && b < max_blocks; b += 8) {
      const unsigned long long* q = &t[(size_t)b * 16];
      if (q[0] == 0) break;
      const unsigned hw = (unsigned)q[8];
      printf("%u.%u.%u ", (hw >> 13) & 7, (hw >> 8) & 0xf, (hw >> 16) & 0xf);
    }
    printf("\n");
  }
  fflush(stdout);
  return 0;
}

// ODT_CONV_TRACE report of odt_op_bottleneck_block (tuning aid): per-phase wall-clock (100 MHz) averages over the tiles
int report_block_trace(Tmp<unsigned long long>& tr, size_t ntile) {
  ODT_HIP(hipDeviceSynchronize());
  std::vector<unsigned long long> t(ntile * 16);
  if (tr.get(t.data(), t.size())) return 1;
  double ph[5] = {0, 0, 0, 0, 0};
  unsigned long long t0 = ~0ull, t1 = 0;
  for (size_t i = 0; i < ntile; ++i) {
    const unsigned long long* q = &t[i * 16];
    ph[0] += (double)(q[1] - q[0]); ph[1] += (double)(q[2] - q[1]); ph[2] += (double)(q[6] - q[2]); ph[3] += (double)(q[3] - q[6]); ph[4] += (double)(q[5] - q[3]);
    if (q[0] < t0) t0 = q[0];
    if (q[5] > t1) t1 = q[5];
  }
  printf("[block trace] tiles=%zu span=%.1f us | per tile avg us: conv1 loop %.2f  patch %.2f  conv2 %.2f  tail pieces %.2f  conv3 + stores %.2f\n",
         ntile, (t1 - t0) / 100.0, ph[0] / ntile / 100, ph[1] / ntile / 100, ph[2] / ntile / 100, ph[3] / ntile / 100, ph[4] / ntile / 100);
  fflush(stdout);
  return 0;
}

// device buffers of the EfficientDet op shims (odt_op_dwconv ... odt_op_preprocess_rgb): every one ends in kGuardBytes of
// sentinel bytes, and GBufs::check() reports -- by the buffer's name -- a launch that wrote into them.  There is no
// sanitizer on the device: this turns a write past the end of an output or scratch buffer into an error of the call.
// Outputs start as sentinel bytes too (an element no kernel wrote reads back as 0x7F7F7F7F, 3.39e38), except where the
// plan zero-initialises the buffer and relies on that (the squeeze-excite gate).
constexpr size_t kGuardBytes = 1024;
constexpr int kGuardByte = 0x7F;

struct GBuf {
  unsigned char* d = nullptr;
  size_t bytes = 0;
  std::string name;
  ~GBuf() { if (d) (void)hipFree(d); }
};

struct GBufs {
  std::vector<std::unique_ptr<GBuf>> v;
  // nbytes payload bytes, payload filled with `fill` (a byte value) or the sentinel (fill < 0), then the guard
  template <typename T>
  int alloc(const char* name, size_t count, T** out, int fill = -1, const void* host = nullptr) {
    v.emplace_back(new GBuf());
    GBuf& g = *v.back();
    g.name = name; g.bytes = count * sizeof(T);
    ODT_HIP(hipMalloc((void**)&g.d, g.bytes + kGuardBytes));
    if (host != nullptr) { ODT_HIP(hipMemcpy(g.d, host, g.bytes, hipMemcpyHostToDevice)); }
    else { ODT_HIP(hipMemset(g.d, fill < 0 ? kGuardByte : fill, g.bytes)); }
    ODT_HIP(hipMemset(g.d + g.bytes, kGuardByte, kGuardBytes));
    *out = reinterpret_cast<T*>(g.d);
    return 0;
  }
  // after the launches: synchronise, then every guard region must still hold the sentinel
  int check(const char* op) {
    ODT_HIP(hipDeviceSynchronize());
    std::vector<unsigned char> h(kGuardBytes);
    for (const auto& g : v) {
      ODT_HIP(hipMemcpy(h.data(), g->d + g->bytes, kGuardBytes, hipMemcpyDeviceToHost));
      for (size_t i = 0; i < kGuardBytes; ++i)
        ODT_CHECK(h[i] == (unsigned char)kGuardByte, std::string(op) + ": write past the end of " + g->name + " (guard byte " +
                                                         std::to_string(i) + ")");
    }
    return 0;
  }
};

template <typename T>
int get_dev(T* host, const T* dev, size_t count) {
  if (host != nullptr && count > 0) ODT_HIP(hipMemcpy(host, dev, count * sizeof(T), hipMemcpyDeviceToHost));
  return 0;
}

// the squeeze-excite gate from per-split partial sums as the plan runs it (OP_SE_GATE_MEAN with a fused squeeze):
// fold + reduce + expand; mean / r scratch start as sentinels, the gate as zeros (pad channels stay 0)
int se_from_parts(GBufs& g, const float* part, int nsplit, int B, int HW, int ldc, int mid, int se, const float* w1,
                  const float* b1, const float* w2t, const float* b2, float** mean, float** gate) {
  ODT_CHECK(w1 && b1 && w2t && b2 && mid >= 1 && mid <= ldc && se >= 1, "squeeze-excite: bad weights / sizes");
  SeGateParams sp; std::memset(&sp, 0, sizeof(sp));
  float *dw1, *db1, *dw2t, *db2;
  if (g.alloc("se_w1", (size_t)se * ldc, &dw1, -1, w1) || g.alloc("se_b1", (size_t)se, &db1, -1, b1) ||
      g.alloc("se_w2t", (size_t)se * ldc, &dw2t, -1, w2t) || g.alloc("se_b2", (size_t)mid, &db2, -1, b2) ||
      g.alloc("se_mean", (size_t)B * ldc, &sp.mean) || g.alloc("se_r", (size_t)B * 256, &sp.r) ||
      g.alloc("se_gate", (size_t)B * ldc, &sp.gate, 0)) return 1;
  sp.part = part; sp.nsplit = nsplit; sp.HW = HW; sp.ldc = ldc; sp.mid = mid; sp.se = se;
  sp.w1 = dw1; sp.b1 = db1; sp.w2t = dw2t; sp.b2 = db2;
  if (launch_se_gate_from_parts(sp, B, nullptr)) return 1;
  *mean = sp.mean; *gate = sp.gate;
  return 0;
}

}  // namespace

extern "C" {

int odt_nn_cosine(int device, const float* gallery, const int32_t* seg_offsets, int T, const float* dets,
                  int N, int D, double* cost) {
  ODT_CHECK(T >= 0 && N >= 0 && D > 0, "odt_nn_cosine: bad sizes");
  if (T == 0 || N == 0) return 0;
  ODT_CHECK(gallery && seg_offsets && dets && cost, "odt_nn_cosine: null argument");
  if (set_dev(device)) return 1;
  const int G = seg_offsets[T];
  ODT_CHECK(G > 0 && seg_offsets[0] == 0, "odt_nn_cosine: bad segment offsets");
  for (int t = 0; t < T; ++t) ODT_CHECK(seg_offsets[t + 1] > seg_offsets[t], "odt_nn_cosine: empty track gallery");
  // persistent per-device scratch + its own stream (no allocation, no null stream, no device-wide sync per call)
  static std::mutex mu;
  static std::map<int, std::unique_ptr<CosineCtx>> ctxs;
  std::lock_guard<std::mutex> lk(mu);
  const int dev = device;
  std::unique_ptr<CosineCtx>& cx = ctxs[dev];
  if (!cx) cx.reset(new CosineCtx());
  std::vector<const float*> gr(G), dr(N);
  for (int g = 0; g < G; ++g) gr[g] = gallery + (size_t)g * D;
  for (int j = 0; j < N; ++j) dr[j] = dets + (size_t)j * D;
  return cx->run(dev, gr.data(), G, seg_offsets, T, dr.data(), N, D, cost);
}

int odt_op_conv2d(int device, const float* in, int B, int H, int W, int Cin, const float* wt_hwio,
                  const float* bias, int kh, int kw, int Cout, int stride, int dil, int pad_t, int pad_l,
                  int Ho, int Wo, int oy, int ox, const float* res, int res_mode, int relu, float* out) {
  ODT_CHECK(in && wt_hwio && out, "odt_op_conv2d: null argument");
  if (set_dev(device)) return 1;
  const size_t nin = (size_t)B * H * W * Cin, nout = (size_t)B * (Ho + oy) * (Wo + ox) * Cout;
  const std::vector<float> w = ohwi(wt_hwio, kh, kw, Cin, Cout), bz(Cout, 0.f);
  const int rH = res_mode == 2 ? (Ho + 1) / 2 : Ho, rW = res_mode == 2 ? (Wo + 1) / 2 : Wo;
  Tmp<float> di, dw, db, dr, dout;
  if (di.alloc(nin) || dw.alloc(w.size()) || db.alloc(Cout) || dout.alloc(nout) || dout.zero()) return 1;
  if (di.put(in) || dw.put(w.data()) || db.put(bias ? bias : bz.data())) return 1;
  if (res && res_mode) { if (dr.alloc((size_t)B * rH * rW * Cout) || dr.put(res)) return 1; }
  ConvParams p = dense_conv(di.d, dw.d, db.d, dout.d, B, H, W, Cin, Ho, Wo, Cout, kh, kw, stride, dil, pad_t, pad_l, relu);
  p.out_H = Ho + oy; p.out_W = Wo + ox; p.out_oy = oy; p.out_ox = ox;
  p.res = (res && res_mode) ? dr.d : nullptr; p.res_mode = p.res ? res_mode : 0; p.res_H = rH; p.res_W = rW; p.res_ldc = Cout;
  Tmp<unsigned long long> tr;
  const Knobs kn = knobs_read();      // (the environment as it is at this call)
  const bool trace = kn.get(K_CONV_TRACE).set;
  const int max_blocks = 1 << 16;
  if (trace) { if (tr.alloc((size_t)max_blocks * 16) || tr.zero()) return 1; p.trace = tr.d; }
  if (run_conv(p, kn)) return 1;      // warm
  if (trace) { if (tr.zero()) return 1; }
  if (run_conv(p, kn)) return 1;
  ODT_HIP(hipDeviceSynchronize());
  if (trace && report_conv_trace(tr, max_blocks)) return 1;
  return dout.get(out, nout);
}

int odt_op_conv2d_cat(int device, const float* a, int B, int Ho, int Wo, int Ca, const float* b2, int Hb,
                      int Wb, int Cb, int stride_b, const float* wa, const float* wb, const float* bias,
                      int Cout, int relu, float* out) {
  ODT_CHECK(a && b2 && wa && wb && out, "odt_op_conv2d_cat: null argument");
  ODT_CHECK((Ho - 1) * stride_b < Hb && (Wo - 1) * stride_b < Wb, "odt_op_conv2d_cat: second input too small");
  if (set_dev(device)) return 1;
  std::vector<float> w((size_t)Cout * (Ca + Cb)), bz(Cout, 0.f);
  for (int o = 0; o < Cout; ++o) {
    for (int i = 0; i < Ca; ++i) w[(size_t)o * (Ca + Cb) + i] = wa[(size_t)i * Cout + o];
    for (int i = 0; i < Cb; ++i) w[(size_t)o * (Ca + Cb) + Ca + i] = wb[(size_t)i * Cout + o];
  }
  Tmp<float> da, db2, dw, dbias, dout;
  const size_t na = (size_t)B * Ho * Wo * Ca, nb = (size_t)B * Hb * Wb * Cb, nout = (size_t)B * Ho * Wo * Cout;
  if (da.alloc(na) || db2.alloc(nb) || dw.alloc(w.size()) || dbias.alloc(Cout) || dout.alloc(nout) || dout.zero()) return 1;
  if (da.put(a) || db2.put(b2) || dw.put(w.data()) || dbias.put(bias ? bias : bz.data())) return 1;
  ConvParams p = same_conv(da.d, dw.d, dbias.d, dout.d, B, Ho, Wo, Ca, Cout, 1, 1, relu);
  p.in2 = db2.d; p.Cin2 = Cb; p.in2_ldc = Cb; p.in2_Ha = Hb; p.in2_Wa = Wb; p.in2_stride = stride_b;
  if (run_conv(p, knobs_read())) return 1;
  ODT_HIP(hipDeviceSynchronize());
  return dout.get(out, nout);
}

// conv2 (3x3, stride 1, 'SAME' for dilation dil, C -> C, bias, ReLU) -> conv3 (1x1, C -> C3, bias (+ residual), ReLU?) on the
// fp16x2 kernels, C = 64 / 128 / 256 (dil 1 or 2, C3 % 64 == 0): fuse = 1 as ONE conv_h2k_kernel launch with the fused tail (the plan's fuse_bottleneck_tails),
// fuse = 0 as the two launches the fused form replaces (conv_h2k_kernel -> [M,C] tensor + recorded range -> conv_h2_kernel).
int odt_op_bottleneck_tail(int device, const float* in, int B, int H, int W, int C, const float* w2_hwio, const float* b2,
                           int dil, const float* w3_io, const float* b3, int C3, const float* res, int relu3, int fuse,
                           float* out) {
  ODT_CHECK(in && w2_hwio && b2 && w3_io && b3 && out, "odt_op_bottleneck_tail: null argument");
  ODT_CHECK((C == 256 || C == 128 || C == 64) && C3 % 64 == 0 && C3 > 0 && (dil == 1 || dil == 2), "odt_op_bottleneck_tail: C = 64 / 128 / 256, C3 % 64 == 0, dil 1 or 2");
  if (set_dev(device)) return 1;
  const size_t M = (size_t)B * H * W;
  const std::vector<float> w2 = ohwi(w2_hwio, 3, 3, C, C), w3 = ohwi(w3_io, 1, 1, C, C3);
  Tmp<float> di, dw2, db2, dw3, db3, dres, dmid, dout, img2, img3, imgf;
  Tmp<unsigned> amax;
  if (di.alloc(M * C) || dw2.alloc(w2.size()) || db2.alloc(C) || dw3.alloc(w3.size()) || db3.alloc(C3) || dmid.alloc(M * C) ||
      dout.alloc(M * C3) || dout.zero() || amax.alloc(4 * kAmaxWays) || amax.zero()) return 1;
  if (di.put(in) || dw2.put(w2.data()) || db2.put(b2) || dw3.put(w3.data()) || db3.put(b3)) return 1;
  if (res) { if (dres.alloc(M * C3) || dres.put(res)) return 1; }
  if (launch_tensor_amax(di.d, M * C, amax.d, nullptr)) return 1;
  unsigned* const slot[3] = {amax.d, amax.d + kAmaxWays, amax.d + 2 * kAmaxWays};      // ranges of in, conv2's and conv3's output
  ConvParams a = same_conv(di.d, dw2.d, db2.d, dmid.d, B, H, W, C, C, 3, dil, 1);
  a.debug = 0x400;
  if (use_h2_row(a, conv_variant_find(CF_H2, 256, C, CVF_KWR), slot[0], slot[1], img2)) return 1;
  ConvParams b = same_conv(dmid.d, dw3.d, db3.d, dout.d, B, H, W, C, C3, 1, 1, relu3 ? 1 : 0);
  b.res = res ? dres.d : nullptr; b.res_mode = res ? 1 : 0; b.res_H = H; b.res_W = W; b.res_ldc = C3; b.debug = 0x400;
  if (use_h2_row(b, C3 % 256 == 0 ? CV_H2_256x256 : (C3 % 128 == 0 ? CV_H2_256x128 : CV_H2_128x64), slot[1], slot[2], img3)) return 1;
  Tmp<ConvParams> rec;
  if (rec.alloc(2)) return 1;
  if (fuse) {
    ODT_CHECK(conv_h2f_fusable(a, b), "odt_op_bottleneck_tail: this pair is not fusable");
    if (imgf.alloc((conv_h2f_weight_bytes(C3, C) + 3) / 4) || conv_make_h2f_weights(dw3.d, C3, C, imgf.d, nullptr)) return 1;
    conv_h2f_fuse(a, b, imgf.d);
    ConvParams recs[2] = {a, b};
    if (conv_check(a) || rec.put(recs)) return 1;
    note_conv(a);
    if (launch_conv(a, rec.d, nullptr)) return 1;
  } else {
    ConvParams recs[2] = {a, b};
    if (conv_check(a) || conv_check(b) || rec.put(recs)) return 1;
    note_conv(b);
    if (launch_conv(a, rec.d, nullptr) || launch_conv(b, rec.d + 1, nullptr)) return 1;
  }
  ODT_HIP(hipDeviceSynchronize());
  return dout.get(out, M * C3);
}

// x -> conv1 (1x1, 4C -> C, ReLU) -> conv2 (3x3 'SAME', ReLU) -> conv3 (1x1, C -> 4C, + x, ReLU) on the fp16x2 kernels, C = 64:
// fuse = 1 as ONE conv_block_kernel launch (the plan's fuse_bottleneck_blocks), fuse = 0 as three launches with both
// intermediate tensors and their recorded ranges.
int odt_op_bottleneck_block(int device, const float* x, int B, int H, int W, int C, const float* w1_io, const float* b1,
                            const float* w2_hwio, const float* b2, const float* w3_io, const float* b3, int fuse, float* out) {
  ODT_CHECK(x && w1_io && b1 && w2_hwio && b2 && w3_io && b3 && out, "odt_op_bottleneck_block: null argument");
  ODT_CHECK(C == 64 && B > 0 && H > 0 && W > 0, "odt_op_bottleneck_block: C = 64");
  if (set_dev(device)) return 1;
  const int C4 = 4 * C;
  const size_t M = (size_t)B * H * W;
  const std::vector<float> w1 = ohwi(w1_io, 1, 1, C4, C), w2 = ohwi(w2_hwio, 3, 3, C, C), w3 = ohwi(w3_io, 1, 1, C, C4);
  Tmp<float> dx, dw1, db1, dw2, db2, dw3, db3, dt1, dt2, dout, img1, img2, img2p, img3, imgf;
  Tmp<unsigned> amax;
  if (dx.alloc(M * C4) || dw1.alloc(w1.size()) || db1.alloc(C) || dw2.alloc(w2.size()) || db2.alloc(C) || dw3.alloc(w3.size()) ||
      db3.alloc(C4) || dt1.alloc(M * C) || dt2.alloc(M * C) || dout.alloc(M * C4) || dout.zero() || amax.alloc(4 * kAmaxWays) || amax.zero()) return 1;
  if (dx.put(x) || dw1.put(w1.data()) || db1.put(b1) || dw2.put(w2.data()) || db2.put(b2) || dw3.put(w3.data()) || db3.put(b3)) return 1;
  if (launch_tensor_amax(dx.d, M * C4, amax.d, nullptr)) return 1;
  unsigned* const slot[4] = {amax.d, amax.d + kAmaxWays, amax.d + 2 * kAmaxWays, amax.d + 3 * kAmaxWays};      // ranges of x, t1, t2, out
  ConvParams c1 = same_conv(dx.d, dw1.d, db1.d, dt1.d, B, H, W, C4, C, 1, 1, 1);
  if (use_h2_row(c1, CV_H2_128x64, slot[0], slot[1], img1)) return 1;
  ConvParams a = same_conv(dt1.d, dw2.d, db2.d, dt2.d, B, H, W, C, C, 3, 1, 1);
  a.debug = 0x400;
  if (use_h2_row(a, conv_variant_find(CF_H2, 256, C, CVF_KWR), slot[1], slot[2], img2)) return 1;
  ConvParams b = same_conv(dt2.d, dw3.d, db3.d, dout.d, B, H, W, C, C4, 1, 1, 1);
  b.res = dx.d; b.res_mode = 1; b.res_H = H; b.res_W = W; b.res_ldc = C4; b.debug = 0x400;
  if (use_h2_row(b, CV_H2_256x256, slot[2], slot[3], img3)) return 1;
  Tmp<ConvParams> rec;
  if (rec.alloc(3)) return 1;
  if (fuse) {
    ODT_CHECK(conv_h2f_fusable(a, b), "odt_op_bottleneck_block: conv2 + conv3 are not fusable");
    if (imgf.alloc((conv_h2f_weight_bytes(C4, C) + 3) / 4) || conv_make_h2f_weights(dw3.d, C4, C, imgf.d, nullptr)) return 1;
    conv_h2f_fuse(a, b, imgf.d);
    ODT_CHECK(conv_block_fits(c1, a), "odt_op_bottleneck_block: this block does not fit conv_block_kernel");
    if (img2p.alloc((conv_split_weight_bytes(C, 9 * C) + 3) / 4) || conv_make_h2p_weights(a, img2p.d, nullptr)) return 1;
    conv_block_fuse(a, c1, img2p.d);      // (t1 does not exist)
    // ODT_CONV_TRACE (tuning): per-phase wall-clock (100 MHz) averages over the workgroups
    const bool trace = knobs_read().get(K_CONV_TRACE).set;
    const size_t ntile = (size_t)B * ((H + 15) / 16) * ((W + 15) / 16);
    Tmp<unsigned long long> tr;
    if (trace) { if (tr.alloc(ntile * 16) || tr.zero()) return 1; a.trace = tr.d; }
    ConvParams recs[3] = {a, c1, b};
    if (conv_check(a) || rec.put(recs)) return 1;
    note_conv(a);
    if (launch_bottleneck_block(a, rec.d, nullptr)) return 1;
    if (trace && report_block_trace(tr, ntile)) return 1;
  } else {
    ConvParams recs[3] = {c1, a, b};
    if (conv_check(c1) || conv_check(a) || conv_check(b) || rec.put(recs)) return 1;
    note_conv(b);
    if (launch_conv(c1, rec.d, nullptr) || launch_conv(a, rec.d + 1, nullptr) || launch_conv(b, rec.d + 2, nullptr)) return 1;
  }
  ODT_HIP(hipDeviceSynchronize());
  return dout.get(out, M * C4);
}

int odt_op_stem(int device, const float* frame_pad, int B, int Hp, int Wp, const float* w_hwio, const float* bias, int fuse,
                int grid, float* out) {
  ODT_CHECK(frame_pad && w_hwio && bias && out && B > 0 && Hp >= 11 && Wp >= 11, "odt_op_stem: null argument / frame too small");
  if (set_dev(device)) return 1;
  const int Ho0 = (Hp - 7) / 2 + 1, Wo0 = (Wp - 7) / 2 + 1, Wa = 2 * Wo0 + 8;      // (room for the 8th, zero-weight tap: plan_fpn.hip)
  const int Hq = (Ho0 + 1 - 3) / 2 + 1, Wq = (Wo0 + 1 - 3) / 2 + 1;
  // the plan's layouts: frames as [B, Hp, Wa, 4] (4th channel and the pad columns zero), conv0 as a 7 x 1 conv over 8-pixel x
  // 4-channel rows: virtual weights [64][7][32]
  std::vector<float> x((size_t)B * Hp * Wa * 4, 0.f), wv((size_t)64 * 7 * 32, 0.f);
  for (int b = 0; b < B; ++b) for (int y = 0; y < Hp; ++y) for (int xx = 0; xx < Wp; ++xx) for (int c = 0; c < 3; ++c)
    x[(((size_t)b * Hp + y) * Wa + xx) * 4 + c] = frame_pad[(((size_t)b * Hp + y) * Wp + xx) * 3 + c];
  for (int y = 0; y < 7; ++y) for (int xx = 0; xx < 7; ++xx) for (int c = 0; c < 3; ++c) for (int o = 0; o < 64; ++o)
    wv[((size_t)o * 7 + y) * 32 + xx * 4 + c] = w_hwio[(((size_t)y * 7 + xx) * 3 + c) * 64 + o];
  Tmp<float> di, dw, db, dmap, dout, img;
  Tmp<unsigned> amax;
  Tmp<ConvParams> rec;
  const size_t nmap = (size_t)B * Ho0 * Wo0 * 64, nout = (size_t)B * Hq * Wq * 64;
  if (di.alloc(x.size()) || dw.alloc(wv.size()) || db.alloc(64) || dmap.alloc(nmap) || dout.alloc(nout) || dout.zero() ||
      amax.alloc(4 * kAmaxWays) || amax.zero() || rec.alloc(1)) return 1;
  if (di.put(x.data()) || dw.put(wv.data()) || db.put(bias)) return 1;
  if (launch_tensor_amax(di.d, x.size(), amax.d, nullptr)) return 1;
  ConvParams p = dense_conv(di.d, dw.d, db.d, dmap.d, B, Hp, Wa, 32, Ho0, Wo0, 64, 7, 1, 2, 1, 0, 0, 1);
  p.in_ldc = 4;      // (Cin = 32: eight 4-channel pixels)
  if (use_h2_row(p, CV_H2_128x64, amax.d, amax.d + kAmaxWays, img)) return 1;
  if (fuse) {
    ODT_CHECK(conv_stem_fits(p), "odt_op_stem: shape not taken by the stem kernel");
    conv_stem_fuse(p, dout.d, Hq, Wq, p.out_ldc);
    if (grid > 0) p.debug |= (grid & 0x3ff) << 20;
    if (conv_check(p) || rec.put(&p)) return 1;
    note_conv(p);
    if (launch_conv(p, rec.d, nullptr)) return 1;
  } else {
    if (conv_check(p) || rec.put(&p)) return 1;
    note_conv(p);
    if (launch_conv(p, rec.d, nullptr)) return 1;
    if (launch_maxpool3x3s2(dmap.d, B, Ho0, Wo0, 64, dout.d, Hq, Wq, nullptr)) return 1;
  }
  ODT_HIP(hipDeviceSynchronize());
  return dout.get(out, nout);
}

// Which kernel would run this conv?  Host only: the record is built from the shape with placeholder (never dereferenced)
// pointers and goes the way of a stand-alone conv call -- conv_check, the policy under the call's knobs, conv_select,
// conv_finish -- up to, not including, the weight image and the launch.  No device is touched.
int odt_op_conv_choice(const int* shape, int conv_arith, int conv_split_family, int* out, char* name, int name_cap) {
  ODT_CHECK(shape && out, "odt_op_conv_choice: null argument");
  static float ph_f[4]; static unsigned ph_u[4];
  for (int i = 0; i < ODT_CONV_CHOICE_OUT; ++i) out[i] = 0;
  if (name && name_cap > 0) name[0] = 0;
  const int* s = shape;
  ConvParams q = dense_conv(ph_f, ph_f, ph_f, ph_f, s[0], s[1], s[2], s[3], s[10], s[11], s[4], s[5], s[6], s[7], s[8], s[9], s[9], 0);
  q.in_Wa = s[12];
  if (s[16] > 0) q.in_ldc = s[16];
  if (s[17] > 0) q.out_ldc = s[17];
  if (s[13] > 0) { q.in2 = ph_f; q.Cin2 = s[13]; q.in2_ldc = s[13]; q.in2_Ha = q.Ho; q.in2_Wa = q.Wo; q.in2_stride = 1; }
  q.res_mode = s[14];
  if (q.res_mode != 0) {
    q.res = ph_f; q.res_ldc = q.out_ldc;
    q.res_H = q.res_mode == 2 ? (q.Ho + 1) / 2 : q.Ho; q.res_W = q.res_mode == 2 ? (q.Wo + 1) / 2 : q.Wo;
  }
  if (s[15]) { q.in_amax = ph_u; if (q.in2 != nullptr) q.in2_amax = ph_u; }
  const Knobs kn = knobs_read();      // (the environment as it is at this call)
  if (conv_check(q)) { out[0] = 2; return 0; }
  ConvPolicy pol = conv_policy_default();      // odt_config first, the knobs on top (resolve_conv_policy)
  if (conv_arith == ODT_ARITH_F32) pol.arith = 0;
  else if (conv_arith == ODT_ARITH_BF16X3) pol.arith = 1;
  if (conv_split_family >= 1 && conv_split_family <= 3) pol.family = conv_split_family;
  pol = conv_policy_with_knobs(pol, kn);
  const ConvChoice ch = conv_select(q, pol, kn);
  if (conv_variant_row(ch.variant).family != CF_F32) {
    conv_use_variant(q, ch.variant, ch.splitk, ch.reduce_blocks);
    q.wt_split = ph_f;
    if (conv_variant_row(q.variant).family == CF_H2) q.h2_chinv = ph_f;
    if (conv_split_partial_bytes(q) > 0) q.partial = ph_f;
  }
  if (conv_finish(q, kn)) { out[0] = 2; return 0; }
  conv_report(q.variant, q.splitk, q.reduce_blocks, out, name, name_cap);
  return 0;
}

// Which kernel did the last stand-alone conv call of this thread launch (odt_op_conv2d, odt_op_conv2d_cat, odt_op_se_tail's
// conv3; odt_op_bottleneck_tail, odt_op_bottleneck_block and odt_op_stem: the LAST conv launch of the call -- the fused record
// with fuse = 1)?  The fields of odt_op_conv_choice, taken from the finished record at its launch point.  Host only.
int odt_op_last_conv(int* out, char* name, int name_cap) {
  ODT_CHECK(out, "odt_op_last_conv: null argument");
  ODT_CHECK(g_last_conv.variant != CV_NONE, "odt_op_last_conv: this thread has launched no stand-alone conv yet");
  conv_report(g_last_conv.variant, g_last_conv.splitk, g_last_conv.reduce_blocks, out, name, name_cap);
  return 0;
}

int odt_op_preprocess(int device, const void* frames, int dtype, int B, int H, int W, int pad_t, int pad_l,
                      int Hp, int Wp, float* out) {
  ODT_CHECK(frames && out, "odt_op_preprocess: null argument");
  if (set_dev(device)) return 1;
  const size_t nin = (size_t)B * H * W * 3 * (dtype == ODT_DTYPE_U8 ? 1 : 4);
  Tmp<unsigned char> di; Tmp<float> dout;
  if (di.alloc(nin) || di.put((const unsigned char*)frames) || dout.alloc((size_t)B * Hp * Wp * 4)) return 1;
  if (launch_preprocess(di.d, dtype, B, H, W, pad_t, pad_l, Hp, Wp, dout.d, nullptr)) return 1;
  ODT_HIP(hipDeviceSynchronize());
  return dout.get(out, dout.n);
}

int odt_op_maxpool(int device, const float* in, int B, int H, int W, int C, float* out) {
  ODT_CHECK(in && out, "odt_op_maxpool: null argument");
  if (set_dev(device)) return 1;
  const int Ho = (H + 1 - 3) / 2 + 1, Wo = (W + 1 - 3) / 2 + 1;
  Tmp<float> di, dout;
  if (di.alloc((size_t)B * H * W * C) || di.put(in) || dout.alloc((size_t)B * Ho * Wo * C)) return 1;
  if (launch_maxpool3x3s2(di.d, B, H, W, C, dout.d, Ho, Wo, nullptr)) return 1;
  ODT_HIP(hipDeviceSynchronize());
  return dout.get(out, dout.n);
}

int odt_op_topk(int device, const float* scores, int n, int k, int32_t* idx_out) {
  ODT_CHECK(scores && idx_out, "odt_op_topk: null argument");
  if (set_dev(device)) return 1;
  Tmp<float> ds; Tmp<int> di;
  if (ds.alloc(n) || ds.put(scores) || di.alloc(k)) return 1;
  if (launch_topk(ds.d, n, k, di.d, nullptr)) return 1;
  ODT_HIP(hipDeviceSynchronize());
  return di.get(idx_out, k);
}

int odt_op_nms(int device, const float* boxes, const float* scores, int n, int max_out, float iou_thresh,
               int32_t* idx_out, int* n_out) {
  ODT_CHECK(idx_out && n_out, "odt_op_nms: null argument");
  if (n == 0) { *n_out = 0; return 0; }
  ODT_CHECK(boxes && scores, "odt_op_nms: null argument");
  if (set_dev(device)) return 1;
  Tmp<float> db, ds; Tmp<int> di, dn;
  if (db.alloc((size_t)n * 4) || db.put(boxes) || ds.alloc(n) || ds.put(scores) || di.alloc(n) || dn.alloc(1)) return 1;
  if (launch_nms(db.d, ds.d, n, max_out, iou_thresh, di.d, dn.d, nullptr)) return 1;
  ODT_HIP(hipDeviceSynchronize());
  if (dn.get(n_out, 1)) return 1;
  return di.get(idx_out, *n_out);
}

int odt_op_proposals(int device, int graph, int B, int L, const int* hs, const int* ws, const int* fields,
                     const float* const* rpn, const float* const* anchors, int img_h, int img_w, int K,
                     float nms_thresh, float decode_clip, float* props, int32_t* nprops) {
  ODT_CHECK(L >= 1 && L <= 5 && hs && ws && fields && rpn && anchors && props && nprops, "odt_op_proposals: bad argument");
  if (set_dev(device)) return 1;
  ProposalParams p; std::memset(&p, 0, sizeof(p));
  Tmp<float> dr[5], da[5];
  for (int l = 0; l < L; ++l) {
    if (dr[l].alloc((size_t)B * hs[l] * ws[l] * kRpnCh) || dr[l].put(rpn[l])) return 1;
    if (da[l].alloc((size_t)fields[l] * fields[l] * 12) || da[l].put(anchors[l])) return 1;
    p.lvl[l].rpn = dr[l].d; p.lvl[l].anchors = da[l].d; p.lvl[l].h = hs[l]; p.lvl[l].w = ws[l]; p.lvl[l].field = fields[l];
  }
  p.nlevels = L; p.graph = graph; p.B = B; p.K = K; p.img_h = img_h; p.img_w = img_w;
  p.nms_thresh = nms_thresh; p.decode_clip = decode_clip;
  const size_t per = (size_t)B * L * K;
  Tmp<float> cb, cs, lb, ls, pr; Tmp<int> cc, lc, np;
  if (cb.alloc(per * 4) || cs.alloc(per) || lb.alloc(per * 4) || ls.alloc(per) || pr.alloc((size_t)B * K * 4) ||
      cc.alloc((size_t)B * L) || lc.alloc((size_t)B * L) || np.alloc(B)) return 1;
  p.cand_boxes = cb.d; p.cand_scores = cs.d; p.lvl_boxes = lb.d; p.lvl_scores = ls.d;
  p.cand_count = cc.d; p.lvl_count = lc.d; p.props = pr.d; p.nprops = np.d;
  Tmp<unsigned long long> ck;
  if (ck.alloc((size_t)B * proposal_total_chunks(p) * K)) return 1;
  p.chunk_keys = ck.d;
  if (launch_proposals(p, nullptr)) return 1;
  ODT_HIP(hipDeviceSynchronize());
  if (pr.get(props, (size_t)B * K * 4)) return 1;
  return np.get(nprops, B);
}

int odt_op_roi_align(int device, int B, int C, const int* hs, const int* ws, const float* const* feats,
                     const float* strides, const float* boxes, const int32_t* box_ind, int R,
                     float* out_nchw, float* pooled) {
  ODT_CHECK(hs && ws && feats && strides && boxes && box_ind && out_nchw, "odt_op_roi_align: null argument");
  if (R == 0) return 0;
  if (set_dev(device)) return 1;
  RoiAlignParams p; std::memset(&p, 0, sizeof(p));
  Tmp<float> df[4], db, dout, dpool; Tmp<int> di;
  for (int l = 0; l < 4; ++l) {
    if (df[l].alloc((size_t)B * hs[l] * ws[l] * C) || df[l].put(feats[l])) return 1;
    p.feat[l] = df[l].d; p.h[l] = p.alloc_h[l] = hs[l]; p.w[l] = p.alloc_w[l] = ws[l]; p.ldc[l] = C;
    p.inv_stride[l] = (float)(1.0 / (double)strides[l]);
  }
  if (db.alloc((size_t)R * 4) || db.put(boxes) || di.alloc(R) || di.put(box_ind) ||
      dout.alloc((size_t)R * C * 49) || dpool.alloc((size_t)R * C)) return 1;
  p.C = C; p.boxes = db.d; p.box_ind = di.d; p.per_image = 0; p.count = nullptr; p.R_cap = R;
  p.out_nchw = dout.d; p.pooled = pooled ? dpool.d : nullptr;
  if (launch_roi_align(p, nullptr)) return 1;
  ODT_HIP(hipDeviceSynchronize());
  if (dout.get(out_nchw, dout.n)) return 1;
  if (pooled) return dpool.get(pooled, dpool.n);
  return 0;
}

int odt_op_roi_align_plan(int device, int B, int C, int L, const int32_t* dims, const float* const* feats, const float* strides,
                          const float* boxes, int per_image, const int32_t* count, const int32_t* levels, int level0,
                          int out_size, int pack_rows, int want_amax, float* out_nhwc, float* out_nchw, float* pooled,
                          uint32_t* amax) {
  ODT_CHECK(dims && feats && strides && boxes, "odt_op_roi_align_plan: null argument");
  ODT_CHECK(B >= 1 && per_image >= 1 && C >= 1 && L >= 1 && L <= 5, "odt_op_roi_align_plan: bad sizes");
  ODT_CHECK(out_size == 0 || out_size == kRoiOut || out_size == 2 * kRoiOut, "odt_op_roi_align_plan: output side must be 7 or 14");
  ODT_CHECK(levels != nullptr || L >= 4, "odt_op_roi_align_plan: the FPN level rule needs four levels");
  const int R = B * per_image, OO = out_size == 2 * kRoiOut ? 4 * kRoiOut * kRoiOut : kRoiOut * kRoiOut;
  for (int l = 0; l < L; ++l) {
    const int32_t* d = dims + 5 * l;      // h, w, alloc_h, alloc_w, ldc
    ODT_CHECK(feats[l] != nullptr && d[0] >= 1 && d[1] >= 1 && d[2] >= d[0] && d[3] >= d[1] && d[4] >= C && strides[l] > 0.f,
              "odt_op_roi_align_plan: a level's view must lie inside its allocation");
  }
  for (int r = 0; levels != nullptr && r < R; ++r)
    ODT_CHECK(levels[r] >= level0 && levels[r] < level0 + L, "odt_op_roi_align_plan: level out of range");
  for (int b = 0; count != nullptr && b < B; ++b)
    ODT_CHECK(count[b] >= 0 && count[b] <= per_image, "odt_op_roi_align_plan: count out of range");
  if (set_dev(device)) return 1;
  GBufs g;
  RoiAlignParams p; std::memset(&p, 0, sizeof(p));
  static const char* names[5] = {"feat0", "feat1", "feat2", "feat3", "feat4"};
  for (int l = 0; l < L; ++l) {
    const int32_t* d = dims + 5 * l;
    float* df;
    if (g.alloc(names[l], (size_t)B * d[2] * d[3] * d[4], &df, -1, feats[l])) return 1;
    p.feat[l] = df; p.h[l] = d[0]; p.w[l] = d[1]; p.alloc_h[l] = d[2]; p.alloc_w[l] = d[3]; p.ldc[l] = d[4];
    p.inv_stride[l] = (float)(1.0 / (double)strides[l]);
  }
  float* dbox; int *dcount = nullptr, *dlev = nullptr;
  if (g.alloc("boxes", (size_t)R * 4, &dbox, -1, boxes)) return 1;
  if (count != nullptr && g.alloc("count", (size_t)B, &dcount, -1, count)) return 1;
  if (levels != nullptr && g.alloc("levels", (size_t)R, &dlev, -1, levels)) return 1;
  if (out_nhwc != nullptr && g.alloc("out_nhwc", (size_t)R * OO * C, &p.out_nhwc)) return 1;
  if (out_nchw != nullptr && g.alloc("out_nchw", (size_t)R * OO * C, &p.out_nchw)) return 1;
  if (pooled != nullptr && g.alloc("pooled", (size_t)R * C, &p.pooled)) return 1;
  if (want_amax && g.alloc("amax", (size_t)1, &p.amax, 0)) return 1;
  p.levels = dlev; p.level0 = level0; p.C = C; p.boxes = dbox; p.box_ind = nullptr; p.per_image = per_image; p.count = dcount;
  p.R_cap = R; p.out_size = out_size; p.pack_rows = pack_rows;
  if (launch_roi_align(p, nullptr)) return 1;
  if (g.check("odt_op_roi_align_plan")) return 1;
  if (get_dev(out_nhwc, p.out_nhwc, (size_t)R * OO * C) || get_dev(out_nchw, p.out_nchw, (size_t)R * OO * C) ||
      get_dev(pooled, p.pooled, (size_t)R * C)) return 1;
  if (want_amax) return get_dev(amax, p.amax, (size_t)1);
  return 0;
}

int odt_op_mask_select(int device, const float* logits, int ld, const int32_t* labels, const int32_t* valid, int B,
                       int per_image, float* masks) {
  ODT_CHECK(logits && labels && valid && masks, "odt_op_mask_select: null argument");
  ODT_CHECK(B >= 1 && per_image >= 1 && ld >= 1, "odt_op_mask_select: bad sizes");
  const int R = B * per_image;
  for (int b = 0; b < B; ++b) {
    ODT_CHECK(valid[b] >= 0 && valid[b] <= per_image, "odt_op_mask_select: valid out of range");
    for (int j = 0; j < valid[b]; ++j)
      ODT_CHECK(labels[b * per_image + j] >= 1 && labels[b * per_image + j] <= ld, "odt_op_mask_select: label out of range");
  }
  if (set_dev(device)) return 1;
  GBufs g;
  MaskSelectParams p; std::memset(&p, 0, sizeof(p));
  float* dlog; int *dlab, *dval;
  if (g.alloc("logits", (size_t)R * 14 * 14 * 4 * ld, &dlog, -1, logits) || g.alloc("labels", (size_t)R, &dlab, -1, labels) ||
      g.alloc("valid", (size_t)B, &dval, -1, valid) || g.alloc("masks", (size_t)R * 784, &p.masks)) return 1;
  p.logits = dlog; p.ld = ld; p.labels = dlab; p.valid = dval; p.B = B; p.per_image = per_image;
  if (launch_mask_select(p, nullptr)) return 1;
  if (g.check("odt_op_mask_select")) return 1;
  return get_dev(masks, p.masks, (size_t)R * 784);
}

int odt_op_detections(int device, int graph, int B, int K, int C, const float* cls_logits,
                      const float* box_logits, const float* props, const int32_t* nprops, int img_h, int img_w,
                      const float* reg_weights, float decode_clip, float score_thresh, float nms_thresh,
                      int per_im, float* boxes, float* probs, int32_t* labels, int32_t* valid) {
  ODT_CHECK(cls_logits && box_logits && props && nprops && reg_weights && boxes && probs && labels && valid,
            "odt_op_detections: null argument");
  if (set_dev(device)) return 1;
  const int rows = B * K, ld = C * 5;
  std::vector<float> ho((size_t)rows * ld);
  for (int r = 0; r < rows; ++r) {
    std::memcpy(&ho[(size_t)r * ld], &cls_logits[(size_t)r * C], sizeof(float) * C);
    std::memcpy(&ho[(size_t)r * ld + C], &box_logits[(size_t)r * C * 4], sizeof(float) * C * 4);
  }
  DetectParams p; std::memset(&p, 0, sizeof(p));
  Tmp<float> dh, dp, dd, dpr, ob, op; Tmp<int> dn, ck, cc, ol, ov;
  if (dh.alloc(ho.size()) || dh.put(ho.data()) || dp.alloc((size_t)rows * 4) || dp.put(props) || dn.alloc(B) ||
      dn.put(nprops) || dd.alloc((size_t)rows * (C - 1) * 4) || dpr.alloc((size_t)rows * C) ||
      ck.alloc((size_t)B * (C - 1) * per_im) || cc.alloc((size_t)B * (C - 1)) || ob.alloc((size_t)B * per_im * 4) ||
      op.alloc((size_t)B * per_im) || ol.alloc((size_t)B * per_im) || ov.alloc(B)) return 1;
  p.graph = graph; p.B = B; p.K = K; p.C = C; p.head_out = dh.d; p.ld = ld; p.props = dp.d; p.nprops = dn.d;
  p.img_h = img_h; p.img_w = img_w;
  for (int i = 0; i < 4; ++i) p.reg_w[i] = reg_weights[i];
  p.decode_clip = decode_clip; p.score_thresh = score_thresh; p.nms_thresh = nms_thresh; p.per_im = per_im;
  p.dec_boxes = dd.d; p.probs = dpr.d; p.cls_keep = ck.d; p.cls_count = cc.d;
  p.out_boxes = ob.d; p.out_probs = op.d; p.out_labels = ol.d; p.out_valid = ov.d;
  if (launch_detections(p, nullptr)) return 1;
  ODT_HIP(hipDeviceSynchronize());
  if (ob.get(boxes, ob.n) || op.get(probs, op.n) || ol.get(labels, ol.n)) return 1;
  return ov.get(valid, B);
}

int odt_op_class_nms(int device, int graph, int B, int N, int C, const float* boxes_in, const float* scores_in,
                     const int32_t* ncand, float score_thresh, float nms_thresh, int per_im, float* boxes,
                     float* scores, int32_t* labels, int32_t* valid) {
  ODT_CHECK(boxes_in && scores_in && ncand && boxes && scores && labels && valid, "odt_op_class_nms: null argument");
  ODT_CHECK(C >= 1 && N >= 1, "odt_op_class_nms: bad sizes");
  if (set_dev(device)) return 1;
  const int rows = B * N, Cp = C + 1;
  std::vector<float> pr((size_t)rows * Cp, 0.f);
  for (int r = 0; r < rows; ++r) std::memcpy(&pr[(size_t)r * Cp + 1], &scores_in[(size_t)r * C], sizeof(float) * C);
  DetectParams p; std::memset(&p, 0, sizeof(p));
  Tmp<float> dd, dpr, ob, op; Tmp<int> dn, ck, cc, ol, ov;
  if (dd.alloc((size_t)rows * C * 4) || dd.put(boxes_in) || dpr.alloc(pr.size()) || dpr.put(pr.data()) || dn.alloc(B) ||
      dn.put(ncand) || ck.alloc((size_t)B * C * per_im) || cc.alloc((size_t)B * C) || ob.alloc((size_t)B * per_im * 4) ||
      op.alloc((size_t)B * per_im) || ol.alloc((size_t)B * per_im) || ov.alloc(B)) return 1;
  p.graph = graph; p.B = B; p.K = N; p.C = Cp; p.nprops = dn.d;
  p.score_thresh = score_thresh; p.nms_thresh = nms_thresh; p.per_im = per_im;
  p.dec_boxes = dd.d; p.probs = dpr.d; p.cls_keep = ck.d; p.cls_count = cc.d;
  p.out_boxes = ob.d; p.out_probs = op.d; p.out_labels = ol.d; p.out_valid = ov.d;
  if (launch_class_nms(p, nullptr)) return 1;
  ODT_HIP(hipDeviceSynchronize());
  if (ob.get(boxes, ob.n) || op.get(scores, op.n) || ol.get(labels, ol.n)) return 1;
  return ov.get(valid, B);
}

int odt_op_dwconv(int device, const float* in, int B, int H, int W, int ldc, const float* wt, const float* bias, int k,
                  int stride, int pad_t, int pad_l, int Ho, int Wo, int act, int nmaps, const int32_t* map_hw, int se,
                  int mid, const float* w1, const float* b1, const float* w2t, const float* b2, float* out, float* mean,
                  float* gate, int32_t* info) {
  ODT_CHECK(in && wt && bias && out, "odt_op_dwconv: null argument");
  ODT_CHECK(ldc > 0 && ldc % 4 == 0 && B >= 1 && nmaps >= 0 && nmaps <= 5 && (act == 0 || act == 2), "odt_op_dwconv: bad sizes");
  ODT_CHECK(nmaps == 0 || (map_hw != nullptr && w1 == nullptr), "odt_op_dwconv: multi-map launches take map sizes and no squeeze");
  if (set_dev(device)) return 1;
  DwConvParams p; std::memset(&p, 0, sizeof(p));
  p.B = B; p.H = H; p.W = W; p.Ho = Ho; p.Wo = Wo; p.ldc = ldc; p.k = k; p.stride = stride; p.pad_t = pad_t; p.pad_l = pad_l;
  p.act = act; p.nlvl = nmaps;
  size_t npix_in = (size_t)B * H * W, npix_out = (size_t)B * Ho * Wo;
  if (nmaps > 0) {
    npix_in = npix_out = 0;
    for (int i = 0; i < nmaps; ++i) {
      ODT_CHECK(map_hw[2 * i] >= 1 && map_hw[2 * i + 1] >= 1, "odt_op_dwconv: empty map");
      p.lH[i] = map_hw[2 * i]; p.lW[i] = map_hw[2 * i + 1];
      npix_in += (size_t)p.lH[i] * p.lW[i];
    }
    npix_out = npix_in;
  }
  const bool squeeze = w1 != nullptr;
  const Knobs kn = knobs_read();      // (the environment as it is at this call)
  if (dwconv_plan(p, squeeze, kn)) return 1;
  GBufs g;
  float *din, *dout;
  const float *dwt, *dbias;
  if (g.alloc("in", npix_in * ldc, &din, -1, in) || g.alloc("wt", (size_t)k * k * ldc, (float**)&dwt, -1, wt) ||
      g.alloc("bias", (size_t)ldc, (float**)&dbias, -1, bias) || g.alloc("out", npix_out * ldc, &dout)) return 1;
  p.in = din; p.wt = dwt; p.bias = dbias; p.out = dout;
  for (size_t i = 0, off = 0; i < (size_t)nmaps; off += (size_t)p.lH[i] * p.lW[i] * ldc, ++i) {
    p.lin[i] = din + off; p.lout[i] = dout + off;
  }
  if (squeeze) {      // sum_part sized from the split count dwconv_plan chose, as the plan sizes it
    ODT_CHECK(p.nsplit >= 1 && p.nsplit <= 1024, "dwconv_plan: bad number of partial sums");
    if (g.alloc("sum_part", (size_t)B * p.nsplit * ldc, &p.sum_part)) return 1;
  }
  if (launch_dwconv(p, nullptr)) return 1;
  float *dmean = nullptr, *dgate = nullptr;
  if (squeeze && se_from_parts(g, p.sum_part, p.nsplit, B, Ho * Wo, ldc, mid, se, w1, b1, w2t, b2, &dmean, &dgate)) return 1;
  if (g.check("odt_op_dwconv")) return 1;
  if (info != nullptr) { info[0] = p.px; info[1] = p.nsplit; info[2] = p.xcd_bands; info[3] = p.cqn; }
  if (get_dev(out, dout, npix_out * ldc)) return 1;
  if (squeeze && (get_dev(mean, dmean, (size_t)B * ldc) || get_dev(gate, dgate, (size_t)B * ldc))) return 1;
  return 0;
}

int odt_op_se_gate(int device, const float* x, int B, int HW, int ldc, int mid, int se, const float* w1, const float* b1,
                   const float* w2t, const float* b2, float* mean, float* gate, float* scaled, int32_t* info) {
  ODT_CHECK(x && w1 && b1 && w2t && b2 && mean && gate, "odt_op_se_gate: null argument");
  ODT_CHECK(B >= 1 && HW >= 1 && ldc > 0 && ldc % 4 == 0 && mid >= 1 && mid <= ldc && se >= 1, "odt_op_se_gate: bad sizes");
  if (set_dev(device)) return 1;
  GBufs g;
  SeGateParams sp; std::memset(&sp, 0, sizeof(sp));
  float *dx, *dw1, *db1, *dw2t, *db2, *scratch;
  const int ns = channel_mean_splits(HW, ldc, B);
  if (g.alloc("x", (size_t)B * HW * ldc, &dx, -1, x) || g.alloc("se_w1", (size_t)se * ldc, &dw1, -1, w1) ||
      g.alloc("se_b1", (size_t)se, &db1, -1, b1) || g.alloc("se_w2t", (size_t)se * ldc, &dw2t, -1, w2t) ||
      g.alloc("se_b2", (size_t)mid, &db2, -1, b2) || g.alloc("channel_sum scratch", (size_t)B * ns * ldc, &scratch) ||
      g.alloc("se_mean", (size_t)B * ldc, &sp.mean) || g.alloc("se_r", (size_t)B * 256, &sp.r) ||
      g.alloc("se_gate", (size_t)B * ldc, &sp.gate, 0)) return 1;
  sp.HW = HW; sp.ldc = ldc; sp.mid = mid; sp.se = se; sp.w1 = dw1; sp.b1 = db1; sp.w2t = dw2t; sp.b2 = db2;
  if (launch_se_gate(dx, sp, B, scratch, nullptr)) return 1;
  if (scaled != nullptr && launch_channel_scale(dx, sp.gate, B, HW, ldc, nullptr)) return 1;
  if (g.check("odt_op_se_gate")) return 1;
  if (info != nullptr) info[0] = ns;
  if (get_dev(mean, sp.mean, (size_t)B * ldc) || get_dev(gate, sp.gate, (size_t)B * ldc)) return 1;
  return get_dev(scaled, dx, (size_t)B * HW * ldc);
}

int odt_op_bifpn_fuse(int device, int n, const float* const* ins, const int32_t* in_hw, const int32_t* mode,
                      const int32_t* pads, const float* wsm, int act, int B, int h, int w, int ldc, float* out) {
  ODT_CHECK(ins && in_hw && mode && out, "odt_op_bifpn_fuse: null argument");
  ODT_CHECK(n >= 1 && n <= 3 && B >= 1 && h >= 1 && w >= 1 && ldc > 0 && ldc % 4 == 0 && (act == 0 || act == 2),
            "odt_op_bifpn_fuse: bad sizes");
  if (set_dev(device)) return 1;
  FuseParams p; std::memset(&p, 0, sizeof(p));
  GBufs g;
  static const char* names[3] = {"in0", "in1", "in2"};
  for (int k = 0; k < n; ++k) {
    const int ih = in_hw[2 * k], iw = in_hw[2 * k + 1];
    ODT_CHECK(ins[k] != nullptr && ih >= 1 && iw >= 1, "odt_op_bifpn_fuse: bad input");
    p.ih[k] = ih; p.iw[k] = iw; p.mode[k] = mode[k]; p.sy[k] = p.sx[k] = 1.f; p.pt[k] = p.pl[k] = 0;
    // (the plan's fuse_input: same size, nearest up-sampling with in / out ratios, 3x3 / s2 'SAME' max pool)
    if (mode[k] == 0) {
      ODT_CHECK(ih == h && iw == w, "odt_op_bifpn_fuse: mode 0 input must have the node's size");
    } else if (mode[k] == 1) {
      ODT_CHECK(ih <= h && iw <= w, "odt_op_bifpn_fuse: mode 1 input must not be larger than the node");
      p.sy[k] = (float)ih / (float)h; p.sx[k] = (float)iw / (float)w;
    } else {
      ODT_CHECK(mode[k] == 2 && pads != nullptr && (ih + 1) / 2 == h && (iw + 1) / 2 == w,
                "odt_op_bifpn_fuse: mode 2 input must be the 3x3 / s2 'SAME' pool of the node's size");
      p.pt[k] = pads[2 * k]; p.pl[k] = pads[2 * k + 1];
    }
    float* d;
    if (g.alloc(names[k], (size_t)B * ih * iw * ldc, &d, -1, ins[k])) return 1;
    p.in[k] = d;
  }
  if (wsm != nullptr) {      // 'fastattn': relu of the WSM scalars, tf.add_n left to right + 0.0001
    for (int k = 0; k < n; ++k) p.wgt[k] = std::max(wsm[k], 0.f);
    float tot = p.wgt[0];
    for (int k = 1; k < n; ++k) tot = tot + p.wgt[k];
    p.denom = tot + 0.0001f; p.weighted = 1;
  }
  p.n = n; p.act = act; p.B = B; p.h = h; p.w = w; p.ldc = ldc;
  if (g.alloc("out", (size_t)B * h * w * ldc, &p.out)) return 1;
  if (launch_bifpn_fuse(p, nullptr)) return 1;
  if (g.check("odt_op_bifpn_fuse")) return 1;
  return get_dev(out, p.out, (size_t)B * h * w * ldc);
}

int odt_op_mbconv_expand_dw(int device, const float* x, int B, int H, int W, int in_ldc, const float* e_wt,
                            const float* e_bias, int mid, int lmid, const float* dw_wt, const float* dw_bias, int k,
                            int stride, int pad_t, int pad_l, int Ho, int Wo, int se, const float* w1, const float* b1,
                            const float* w2t, const float* b2, float* out, float* mean, float* gate, int32_t* info) {
  ODT_CHECK(x && e_wt && e_bias && dw_wt && dw_bias && out, "odt_op_mbconv_expand_dw: null argument");
  ODT_CHECK(B >= 1 && H >= 1 && W >= 1 && Ho >= 1 && Wo >= 1 && mid >= 1 && mid <= lmid, "odt_op_mbconv_expand_dw: bad sizes");
  if (set_dev(device)) return 1;
  GBufs g;
  MbExpandDwParams q; std::memset(&q, 0, sizeof(q));
  float *dx, *dew, *deb, *ddw, *ddb, *img;
  if (g.alloc("x", (size_t)B * H * W * in_ldc, &dx, -1, x) || g.alloc("e_wt", (size_t)mid * in_ldc, &dew, -1, e_wt) ||
      g.alloc("e_bias", (size_t)mid, &deb, -1, e_bias) || g.alloc("dw_wt", (size_t)k * k * lmid, &ddw, -1, dw_wt) ||
      g.alloc("dw_bias", (size_t)lmid, &ddb, -1, dw_bias) ||
      g.alloc("w_img", (mbconv_expand_weight_bytes(lmid, in_ldc) + 3) / 4, &img) ||
      g.alloc("out", (size_t)B * Ho * Wo * lmid, &q.out)) return 1;
  {   // the expand weights as the bf16x3 piece image of the one-stage 256 x 64 kernel (plan_effdet.hip, fused MBConv)
    ConvParams cp; std::memset(&cp, 0, sizeof(cp));
    cp.wt = dew; cp.Cout = mid; cp.Cin = in_ldc; cp.kh = 1; cp.kw = 1; conv_use_variant(cp, CV_SPLIT1_256x64);
    if (conv_make_split_weights(cp, img, nullptr)) return 1;
  }
  q.x = dx; q.B = B; q.H = H; q.W = W; q.in_ldc = in_ldc; q.w_img = img; q.e_bias = deb; q.mid = mid; q.lmid = lmid;
  q.dw_wt = ddw; q.dw_bias = ddb; q.Ho = Ho; q.Wo = Wo; q.k = k; q.stride = stride; q.pad_t = pad_t; q.pad_l = pad_l;
  q.nsplit = 0;
  q.nsplit = mbconv_expand_dw_splits(q);
  const bool squeeze = w1 != nullptr;
  if (squeeze && g.alloc("sum_part", (size_t)B * q.nsplit * lmid, &q.sum_part)) return 1;
  if (launch_mbconv_expand_dw(q, nullptr)) return 1;
  float *dmean = nullptr, *dgate = nullptr;
  if (squeeze && se_from_parts(g, q.sum_part, q.nsplit, B, Ho * Wo, lmid, mid, se, w1, b1, w2t, b2, &dmean, &dgate)) return 1;
  if (g.check("odt_op_mbconv_expand_dw")) return 1;
  if (info != nullptr) info[0] = q.nsplit;
  if (get_dev(out, q.out, (size_t)B * Ho * Wo * lmid)) return 1;
  if (squeeze && (get_dev(mean, dmean, (size_t)B * lmid) || get_dev(gate, dgate, (size_t)B * lmid))) return 1;
  return 0;
}

// ---- SE-ResNet bottleneck (resnet_se.hip) ----------------------------------------------------------------------------
namespace {

// device copies of the gate's weights + its scratch, as the plan lays them out (gate rows zero-initialised)
int rse_gate_bufs(GBufs& g, ResSeParams& gp, int B, int HW, int ch, int r, int cout, const float* w1, const float* b1,
                  const float* w2t, const float* b2) {
  std::memset(&gp, 0, sizeof(gp));
  gp.B = B; gp.HW = HW; gp.ch = ch; gp.r = r; gp.cout = cout; gp.gate_ld = (cout + 3) / 4 * 4;
  float *dw1, *db1, *dw2, *db2;
  if (g.alloc("rse_w1", (size_t)r * ch, &dw1, -1, w1) || g.alloc("rse_b1", (size_t)r, &db1, -1, b1) ||
      g.alloc("rse_w2t", (size_t)r * cout, &dw2, -1, w2t) || g.alloc("rse_b2", (size_t)cout, &db2, -1, b2) ||
      g.alloc("rse_part", (size_t)B * channel_mean_splits(HW, ch, B) * ch, &gp.part) ||
      g.alloc("rse_mean", (size_t)B * ch, &gp.mean) || g.alloc("rse_rvec", (size_t)B * r, &gp.rvec) ||
      g.alloc("rse_gate", (size_t)B * gp.gate_ld, &gp.gate, 0)) return 1;
  gp.w1 = dw1; gp.b1 = db1; gp.w2t = dw2; gp.b2 = db2;
  return 0;
}

int rse_read_amax(const unsigned* slot, float* amax) {
  unsigned bits[kAmaxWays], a = 0u;
  ODT_HIP(hipMemcpy(bits, slot, sizeof(bits), hipMemcpyDeviceToHost));
  for (unsigned b : bits) a = b > a ? b : a;
  std::memcpy(amax, &a, 4);
  return 0;
}

}  // namespace

int odt_op_rse_gate(int device, const float* t2, int B, int HW, int ch, int r, int cout, const float* w1, const float* b1,
                    const float* w2t, const float* b2, float* mean, float* gate) {
  ODT_CHECK(t2 && w1 && b1 && w2t && b2 && mean && gate, "odt_op_rse_gate: null argument");
  ODT_CHECK(B >= 1 && HW >= 1 && ch >= 4 && ch % 4 == 0 && r >= 1 && cout >= 1, "odt_op_rse_gate: bad sizes");
  if (set_dev(device)) return 1;
  GBufs g;
  ResSeParams gp;
  float* dt2;
  if (g.alloc("t2", (size_t)B * HW * ch, &dt2, -1, t2) || rse_gate_bufs(g, gp, B, HW, ch, r, cout, w1, b1, w2t, b2)) return 1;
  gp.t2 = dt2;
  if (launch_resnet_se_gate(gp, nullptr)) return 1;
  if (g.check("odt_op_rse_gate")) return 1;
  if (get_dev(mean, gp.mean, (size_t)B * ch)) return 1;
  for (int b = 0; b < B; ++b)
    if (get_dev(gate + (size_t)b * cout, gp.gate + (size_t)b * gp.gate_ld, (size_t)cout)) return 1;
  return 0;
}

int odt_op_rse_apply(int device, const float* y, const float* gate, const float* shortcut, int B, int HW, int C, int ldc,
                     int in_place, float* out, float* amax) {
  ODT_CHECK(y && gate && shortcut && out && amax, "odt_op_rse_apply: null argument");
  ODT_CHECK(B >= 1 && HW >= 1 && C >= 1 && ldc >= C && ldc % 4 == 0, "odt_op_rse_apply: bad sizes");
  if (set_dev(device)) return 1;
  GBufs g;
  ResSeApplyParams ap; std::memset(&ap, 0, sizeof(ap));
  const size_t n = (size_t)B * HW * ldc;
  float *dy, *ds, *dg, *dout;
  unsigned* slot;
  // (gate [B, ldc]; out starts as a copy of the caller's buffer: the channels [C, ldc) must come back as they went in)
  if (g.alloc("y", n, &dy, -1, y) || g.alloc("shortcut", n, &ds, -1, shortcut) || g.alloc("gate", (size_t)B * ldc, &dg, -1, gate) ||
      g.alloc("out", n, &dout, -1, out) || g.alloc("range slot", (size_t)kAmaxWays, &slot, 0)) return 1;
  ap.y = dy; ap.sc = ds; ap.gate = dg; ap.out = in_place ? dy : dout; ap.amax = slot;
  ap.B = B; ap.HW = HW; ap.C = C; ap.ldc = ldc; ap.gate_ld = ldc;
  if (launch_resnet_se_apply(ap, nullptr)) return 1;
  if (g.check("odt_op_rse_apply")) return 1;
  if (rse_read_amax(slot, amax)) return 1;
  return get_dev(out, ap.out, n);
}

int odt_op_se_tail(int device, const float* t2, int B, int H, int W, int ch, const float* w3, const float* b3, const float* w1,
                   const float* b1, const float* w2t, const float* b2, const float* shortcut, float* out, float* gate,
                   float* amax) {
  ODT_CHECK(t2 && w3 && b3 && w1 && b1 && w2t && b2 && shortcut && out && gate && amax, "odt_op_se_tail: null argument");
  ODT_CHECK(B >= 1 && H >= 1 && W >= 1 && ch >= 32 && ch % 32 == 0, "odt_op_se_tail: ch must be a multiple of 32");
  if (set_dev(device)) return 1;
  const int C3 = ch * 4, r = ch / 4, HW = H * W;
  const size_t M = (size_t)B * HW;
  const std::vector<float> w3t = ohwi(w3, 1, 1, ch, C3);
  GBufs g;
  ResSeParams gp;
  float *dt2, *dw3, *db3, *ds, *dy, *dout;
  unsigned* slot;
  if (g.alloc("t2", M * ch, &dt2, -1, t2) || g.alloc("w3", w3t.size(), &dw3, -1, w3t.data()) || g.alloc("b3", (size_t)C3, &db3, -1, b3) ||
      g.alloc("shortcut", M * C3, &ds, -1, shortcut) || g.alloc("y", M * C3, &dy) || g.alloc("out", M * C3, &dout) ||
      g.alloc("range slot", (size_t)kAmaxWays, &slot, 0) || rse_gate_bufs(g, gp, B, HW, ch, r, C3, w1, b1, w2t, b2)) return 1;
  gp.t2 = dt2;
  // the plan's order: pool + gate, conv3 (BN folded, no residual, no ReLU), apply
  if (launch_resnet_se_gate(gp, nullptr)) return 1;
  if (run_conv(same_conv(dt2, dw3, db3, dy, B, H, W, ch, C3, 1, 1, 0), knobs_read())) return 1;
  ResSeApplyParams ap; std::memset(&ap, 0, sizeof(ap));
  ap.y = dy; ap.sc = ds; ap.gate = gp.gate; ap.out = dout; ap.amax = slot;
  ap.B = B; ap.HW = HW; ap.C = C3; ap.ldc = C3; ap.gate_ld = gp.gate_ld;
  if (launch_resnet_se_apply(ap, nullptr)) return 1;
  if (g.check("odt_op_se_tail")) return 1;
  if (rse_read_amax(slot, amax)) return 1;
  if (get_dev(gate, gp.gate, (size_t)B * C3)) return 1;
  return get_dev(out, dout, M * C3);
}

int odt_op_group_conv(int device, const float* x, int B, int H, int W, int C, const float* w, const float* bias, int stride,
                      int dil, int pad_t, int pad_l, int Ho, int Wo, int relu, float* out, float* amax) {
  ODT_CHECK(x && w && bias && out && amax, "odt_op_group_conv: null argument");
  ODT_CHECK(B >= 1 && H >= 1 && W >= 1 && Ho >= 1 && Wo >= 1, "odt_op_group_conv: bad sizes");
  ODT_CHECK(C == 128 || C == 256 || C == 512 || C == 1024, "odt_op_group_conv: C must be 128, 256, 512 or 1024");
  if (set_dev(device)) return 1;
  std::vector<float> img(group_conv_weight_elems(C));
  if (group_conv_pack_weights(w, nullptr, C, img.data())) return 1;
  GBufs g;
  GroupConvParams p; std::memset(&p, 0, sizeof(p));
  const size_t nin = (size_t)B * H * W * C, nout = (size_t)B * Ho * Wo * C;
  float *dx, *dw, *db, *dout;
  unsigned* slot;
  if (g.alloc("x", nin, &dx, -1, x) || g.alloc("w", img.size(), &dw, -1, img.data()) || g.alloc("bias", (size_t)C, &db, -1, bias) ||
      g.alloc("out", nout, &dout) || g.alloc("range slot", (size_t)kAmaxWays, &slot, 0)) return 1;
  p.in = dx; p.wt = dw; p.bias = db; p.out = dout; p.out_amax = slot;
  p.B = B; p.H = H; p.W = W; p.C = C; p.Ho = Ho; p.Wo = Wo; p.stride = stride; p.dil = dil; p.pad_t = pad_t; p.pad_l = pad_l;
  p.relu = relu ? 1 : 0;
  if (launch_group_conv(p, nullptr)) return 1;
  if (g.check("odt_op_group_conv")) return 1;
  if (rse_read_amax(slot, amax)) return 1;
  return get_dev(out, dout, nout);
}

int odt_op_deform_conv(int device, const float* x, int B, int H, int W, int C, const float* w_off, const float* b_off, const float* w,
                       float* out, float* out_amax, float* offsets_out) {
  return odt_op_deform_conv_view(device, x, B, H, W, C, H, W, C, w_off, b_off, w, out, out_amax, offsets_out);
}

int odt_op_deform_conv_view(int device, const float* x, int B, int Ha, int Wa, int ldc, int H, int W, int C, const float* w_off,
                            const float* b_off, const float* w, float* out, float* out_amax, float* offsets_out) {
  ODT_CHECK(x && w_off && b_off && w && out && out_amax && offsets_out, "odt_op_deform_conv: null argument");
  ODT_CHECK(B >= 1 && H >= 1 && W >= 1 && Ha >= H && Wa >= W && ldc >= C && ldc % 4 == 0, "odt_op_deform_conv: bad sizes");
  ODT_CHECK(C == 128 || C == 256 || C == 512, "odt_op_deform_conv: C must be 128, 256 or 512");
  if (set_dev(device)) return 1;
  std::vector<float> io(deform_offset_weight_elems(C)), iw(deform_weight_elems(C));
  if (deform_pack_offset_weights(w_off, C, io.data()) || deform_pack_weights(w, C, iw.data())) return 1;
  GBufs g;
  DeformConvParams p; std::memset(&p, 0, sizeof(p));
  const int Ho = (H + 1) / 2, Wo = (W + 1) / 2;
  const size_t nin = (size_t)B * Ha * Wa * ldc, npx = (size_t)B * Ho * Wo;
  float *dx, *dwo, *dbo, *dw, *doff, *dout;
  unsigned* slot;
  if (g.alloc("x", nin, &dx, -1, x) || g.alloc("w_off", io.size(), &dwo, -1, io.data()) || g.alloc("b_off", (size_t)18, &dbo, -1, b_off) ||
      g.alloc("w", iw.size(), &dw, -1, iw.data()) || g.alloc("offsets", npx * 18, &doff) || g.alloc("out", npx * C, &dout) ||
      g.alloc("range slot", (size_t)kAmaxWays, &slot, 0)) return 1;
  p.in = dx; p.wt_off = dwo; p.b_off = dbo; p.wt = dw; p.off = doff; p.out = dout; p.out_amax = slot;
  p.B = B; p.H = H; p.W = W; p.Ha = Ha; p.Wa = Wa; p.ldc = ldc; p.C = C; p.Ho = Ho; p.Wo = Wo;
  if (launch_deform_conv(p, nullptr)) return 1;
  if (g.check("odt_op_deform_conv")) return 1;
  if (rse_read_amax(slot, out_amax)) return 1;
  if (get_dev(offsets_out, doff, npx * 18)) return 1;
  return get_dev(out, dout, npx * C);
}

int odt_op_group_norm(int device, const float* x, int B, int Ha, int Wa, int ldc, int h, int w, int C, int oy, int ox,
                      const float* gamma, const float* beta, float eps, int relu, int res_mode, const float* res, int res_H,
                      int res_W, int chunks, float* out, float* amax, float* mean, float* var) {
  ODT_CHECK(x && gamma && beta && out && amax && mean && var && (res_mode == 0 || res), "odt_op_group_norm: null argument");
  ODT_CHECK(B >= 1 && Ha >= 1 && Wa >= 1 && ldc >= 1 && h >= 1 && w >= 1 && C >= 1 && (res_mode == 0 || (res_H >= 1 && res_W >= 1)),
            "odt_op_group_norm: bad sizes");
  ODT_CHECK(C % kGnGroups == 0, "odt_op_group_norm: C must be a multiple of 32 (32 groups)");
  if (set_dev(device)) return 1;
  GBufs g;
  GroupNormParams p; std::memset(&p, 0, sizeof(p));
  const size_t n = (size_t)B * Ha * Wa * ldc;
  float *dx, *dg, *db, *dres = nullptr, *dout;
  unsigned* slot;
  // (out starts as a copy of the caller's buffer: what lies outside the view must come back as it went in)
  if (g.alloc("x", n, &dx, -1, x) || g.alloc("gamma", (size_t)C, &dg, -1, gamma) || g.alloc("beta", (size_t)C, &db, -1, beta) ||
      g.alloc("out", n, &dout, -1, out) || g.alloc("range slot", (size_t)kAmaxWays, &slot, 0) ||
      g.alloc("ab", (size_t)B * 2 * C, &p.ab) || g.alloc("mean", (size_t)B * kGnGroups, &p.mean) || g.alloc("var", (size_t)B * kGnGroups, &p.var)) return 1;
  if (res_mode != 0 && g.alloc("res", (size_t)B * res_H * res_W * C, &dres, -1, res)) return 1;
  // (the launcher checks chunks against h; an allocation sized from a bad value must not come first)
  const int parts = group_norm_parts(h, w, C, chunks >= 1 && chunks <= h ? chunks : 0);
  if (g.alloc("part", (size_t)B * kGnGroups * parts * 2, &p.part)) return 1;
  p.x = dx; p.gamma = dg; p.beta = db; p.res = dres; p.out = dout; p.amax = slot;
  p.B = B; p.h = h; p.w = w; p.C = C; p.Ha = Ha; p.Wa = Wa; p.ldc = ldc; p.xoy = oy; p.xox = ox;
  p.oH = Ha; p.oW = Wa; p.out_ldc = ldc; p.oy = oy; p.ox = ox;
  p.res_mode = res_mode; p.res_H = res_H; p.res_W = res_W; p.res_ldc = C; p.relu = relu ? 1 : 0; p.eps = eps; p.chunks = chunks;
  if (launch_group_norm(p, nullptr)) return 1;
  if (g.check("odt_op_group_norm")) return 1;
  if (rse_read_amax(slot, amax)) return 1;
  if (get_dev(mean, p.mean, (size_t)B * kGnGroups) || get_dev(var, p.var, (size_t)B * kGnGroups)) return 1;
  return get_dev(out, dout, n);
}

int odt_op_group_norm_roi(int device, const float* x, int R, int h, int w, int ldc, int C, const float* gamma, const float* beta,
                          float eps, float* out, float* amax, float* mean, float* var) {
  ODT_CHECK(x && gamma && beta && out && amax && mean && var, "odt_op_group_norm_roi: null argument");
  ODT_CHECK(R >= 1 && h >= 1 && w >= 1 && ldc >= 1 && C >= 1 && (double)R * h * w * ldc < 1073741824.0, "odt_op_group_norm_roi: bad sizes");
  if (set_dev(device)) return 1;
  GBufs g;
  RoiGroupNormParams p; std::memset(&p, 0, sizeof(p));
  const size_t n = (size_t)R * h * w * ldc;
  float *dx, *dg, *db, *dout;
  unsigned* slot;
  // (out starts as a copy of the caller's buffer: the pad channels must come back as they went in)
  if (g.alloc("x", n, &dx, -1, x) || g.alloc("gamma", (size_t)C, &dg, -1, gamma) || g.alloc("beta", (size_t)C, &db, -1, beta) ||
      g.alloc("out", n, &dout, -1, out) || g.alloc("range slot", (size_t)kAmaxWays, &slot, 0) ||
      g.alloc("mean", (size_t)R * kGnGroups, &p.mean) || g.alloc("var", (size_t)R * kGnGroups, &p.var)) return 1;
  p.x = dx; p.gamma = dg; p.beta = db; p.out = dout; p.amax = slot;
  p.R = R; p.hw = h * w; p.C = C; p.ldc = ldc; p.out_ldc = ldc; p.eps = eps;
  if (launch_group_norm_roi(p, nullptr)) return 1;
  if (g.check("odt_op_group_norm_roi")) return 1;
  if (rse_read_amax(slot, amax)) return 1;
  if (get_dev(mean, p.mean, (size_t)R * kGnGroups) || get_dev(var, p.var, (size_t)R * kGnGroups)) return 1;
  return get_dev(out, dout, n);
}

int odt_op_relation_geo(int device, const float* boxes, int K, int n, const float* wts, float* bias) {
  ODT_CHECK(boxes && wts && bias, "odt_op_relation_geo: null argument");
  ODT_CHECK(K >= 1, "odt_op_relation_geo: bad sizes");
  ODT_CHECK(K <= kRelMaxK, "odt_op_relation_geo: at most " + std::to_string(kRelMaxK) + " proposals (K = " + std::to_string(K) + ")");
  ODT_CHECK(n >= 0 && n <= K, "odt_op_relation_geo: the proposal count n = " + std::to_string(n) + " is not in [0, K = " + std::to_string(K) + "]");
  if (set_dev(device)) return 1;
  GBufs g;
  RelationGeoParams p; std::memset(&p, 0, sizeof(p));
  const int Kp = relation_kp(K);
  const size_t nb = (size_t)kRelHeads * K * Kp;
  float *db, *dw, *dbias;
  int* dn;
  // (bias starts as a copy of the caller's buffer: what the kernel does not evaluate must come back as it went in)
  if (g.alloc("boxes", (size_t)K * 4, &db, -1, boxes) || g.alloc("weights", (size_t)kRelGeoWeights, &dw, -1, wts) ||
      g.alloc("count", (size_t)1, &dn, -1, &n) || g.alloc("bias", nb, &dbias, -1, bias)) return 1;
  p.boxes = db; p.count = dn; p.wts = dw; p.bias = dbias; p.B = 1; p.K = K; p.Kp = Kp;
  if (launch_relation_geo(p, nullptr)) return 1;
  if (g.check("odt_op_relation_geo")) return 1;
  return get_dev(bias, dbias, nb);
}

int odt_op_relation_attention(int device, const float* q, const float* k, const float* v, const float* bias, int K, int D, int n,
                              float* out, size_t out_elems, float* amax) {
  ODT_CHECK(q && k && v && bias && out && amax, "odt_op_relation_attention: null argument");
  ODT_CHECK(K >= 1 && D >= 1, "odt_op_relation_attention: bad sizes");
  ODT_CHECK(K <= kRelMaxK, "odt_op_relation_attention: at most " + std::to_string(kRelMaxK) + " proposals (K = " + std::to_string(K) + ")");
  ODT_CHECK(D % 64 == 0 && D <= kRelMaxD,
            "odt_op_relation_attention: D must be a multiple of 64 in [64, " + std::to_string(kRelMaxD) + "] (D = " + std::to_string(D) + ")");
  ODT_CHECK(n >= 0 && n <= K, "odt_op_relation_attention: the proposal count n = " + std::to_string(n) + " is not in [0, K = " + std::to_string(K) + "]");
  ODT_CHECK(out_elems >= (size_t)K * kRelHeads * D, "odt_op_relation_attention: out is smaller than [K,16,D]");
  if (set_dev(device)) return 1;
  GBufs g;
  RelationAttnParams p; std::memset(&p, 0, sizeof(p));
  const int Kp = relation_kp(K);
  float *dq, *dk, *dv, *dbias, *dout;
  int* dn;
  unsigned* slot;
  if (g.alloc("q", (size_t)K * D, &dq, -1, q) || g.alloc("k", (size_t)K * D, &dk, -1, k) || g.alloc("v", (size_t)K * D, &dv, -1, v) ||
      g.alloc("bias", (size_t)kRelHeads * K * Kp, &dbias, -1, bias) || g.alloc("count", (size_t)1, &dn, -1, &n) ||
      g.alloc("out", out_elems, &dout, -1, out) || g.alloc("range slot", (size_t)kAmaxWays, &slot, 0)) return 1;
  p.q = dq; p.k = dk; p.v = dv; p.bias = dbias; p.count = dn; p.out = dout; p.amax = slot;
  p.B = 1; p.K = K; p.Kp = Kp; p.D = D; p.qk_ldc = D; p.v_ldc = D;
  if (launch_relation_attention(p, nullptr)) return 1;
  if (g.check("odt_op_relation_attention")) return 1;
  if (rse_read_amax(slot, amax)) return 1;
  return get_dev(out, dout, out_elems);
}

int odt_op_effdet_post(int device, int B, int ncls, const int32_t* npix, int ldc_cls, int ldc_box,
                       const float* const* cls, const float* const* box, const float* anchors, int k, int max_out,
                       float score_thresh, float iou_thresh, float image_scale, int32_t* cand_idx, float* cand_boxes,
                       float* cand_scores, int32_t* cand_cls, int32_t* cand_lvl, float* boxes, float* scores,
                       int32_t* labels, int32_t* levels, int32_t* valid) {
  ODT_CHECK(npix && cls && box && anchors && boxes && scores && labels && levels && valid, "odt_op_effdet_post: null argument");
  ODT_CHECK(B >= 1 && ncls >= 1 && ldc_cls >= 9 * ncls && ldc_box >= 36, "odt_op_effdet_post: bad sizes");
  if (set_dev(device)) return 1;
  EffPostParams p; std::memset(&p, 0, sizeof(p));
  GBufs g;
  static const char* cn[5] = {"cls3", "cls4", "cls5", "cls6", "cls7"};
  static const char* bn[5] = {"box3", "box4", "box5", "box6", "box7"};
  int tot = 0;
  for (int l = 0; l < 5; ++l) {
    ODT_CHECK(npix[l] >= 1 && cls[l] && box[l], "odt_op_effdet_post: bad level");
    float *dc, *db;
    if (g.alloc(cn[l], (size_t)B * npix[l] * ldc_cls, &dc, -1, cls[l]) ||
        g.alloc(bn[l], (size_t)B * npix[l] * ldc_box, &db, -1, box[l])) return 1;
    p.cls[l] = dc; p.box[l] = db; p.npix[l] = npix[l]; p.anchor_off[l] = tot; tot += npix[l] * 9;
  }
  p.anchor_off[5] = tot;
  p.ldc_cls = ldc_cls; p.ldc_box = ldc_box; p.ncls = ncls; p.B = B; p.k = k; p.max_out = max_out;
  p.score_thresh = score_thresh; p.iou_thresh = iou_thresh; p.image_scale = image_scale;
  const size_t nlog = (size_t)tot * ncls;
  float* da;
  if (g.alloc("anchors", (size_t)tot * 4, &da, -1, anchors) || g.alloc("keys", nlog, &p.keys) ||
      g.alloc("hist", 256, &p.hist, 0) || g.alloc("state", 5, &p.state, 0) || g.alloc("sel", (size_t)B * k, &p.sel) ||
      g.alloc("cand_boxes", (size_t)B * k * 4, &p.cand_boxes) || g.alloc("cand_scores", (size_t)B * k, &p.cand_scores) ||
      g.alloc("cand_cls", (size_t)B * k, &p.cand_cls) || g.alloc("cand_lvl", (size_t)B * k, &p.cand_lvl) ||
      g.alloc("out_boxes", (size_t)B * max_out * 4, &p.out_boxes) || g.alloc("out_scores", (size_t)B * max_out, &p.out_scores) ||
      g.alloc("out_labels", (size_t)B * max_out, &p.out_labels) || g.alloc("out_levels", (size_t)B * max_out, &p.out_levels) ||
      g.alloc("out_valid", (size_t)B, &p.out_valid)) return 1;
  p.anchors = da;
  if (launch_effdet_post(p, nullptr)) return 1;
  if (g.check("odt_op_effdet_post")) return 1;
  {   // every one of the k slots per image must hold a selected key (a slot the compaction missed decodes as class -1)
    std::vector<int32_t> cc((size_t)B * k);
    if (get_dev(cc.data(), p.cand_cls, cc.size())) return 1;
    for (size_t i = 0; i < cc.size(); ++i)
      ODT_CHECK(cc[i] >= 0 && cc[i] < ncls, "odt_op_effdet_post: top-k slot " + std::to_string(i % k) + " of image " +
                                                std::to_string(i / k) + " was not filled by the selection");
  }
  if (cand_idx != nullptr) {      // the selected (anchor * ncls + class) indices, sorted here by their keys: the set in reference order
    std::vector<unsigned long long> sel((size_t)B * k);
    if (get_dev(sel.data(), p.sel, sel.size())) return 1;
    for (int b = 0; b < B; ++b) {
      std::sort(sel.begin() + (size_t)b * k, sel.begin() + (size_t)(b + 1) * k, std::greater<unsigned long long>());
      for (int i = 0; i < k; ++i) cand_idx[(size_t)b * k + i] = (int32_t)(0xFFFFFFFFu - (unsigned)sel[(size_t)b * k + i]);
    }
  }
  if (get_dev(cand_boxes, p.cand_boxes, (size_t)B * k * 4) || get_dev(cand_scores, p.cand_scores, (size_t)B * k) ||
      get_dev(cand_cls, p.cand_cls, (size_t)B * k) || get_dev(cand_lvl, p.cand_lvl, (size_t)B * k)) return 1;
  if (get_dev(boxes, p.out_boxes, (size_t)B * max_out * 4) || get_dev(scores, p.out_scores, (size_t)B * max_out) ||
      get_dev(labels, p.out_labels, (size_t)B * max_out) || get_dev(levels, p.out_levels, (size_t)B * max_out)) return 1;
  return get_dev(valid, p.out_valid, (size_t)B);
}

int odt_op_preprocess_rgb(int device, const void* frames, int dtype, int B, int Hs, int Ws, int Hr, int Wr, int pad_t,
                          int pad_l, int Hp, int Wp, int resize, float* out) {
  ODT_CHECK(frames && out, "odt_op_preprocess_rgb: null argument");
  ODT_CHECK(dtype == ODT_DTYPE_U8 || dtype == ODT_DTYPE_F32, "preprocess: dtype must be ODT_DTYPE_U8 or ODT_DTYPE_F32");
  ODT_CHECK(B >= 1 && Hs >= 1 && Ws >= 1 && Hp >= 1 && Wp >= 1 && (!resize || (Hr >= 1 && Wr >= 1)), "odt_op_preprocess_rgb: bad sizes");
  if (set_dev(device)) return 1;
  GBufs g;
  unsigned char* df;
  float* dout;
  if (g.alloc("frames", (size_t)B * Hs * Ws * 3 * (dtype == ODT_DTYPE_U8 ? 1 : 4), &df, -1, frames) ||
      g.alloc("out", (size_t)B * Hp * Wp * 4, &dout)) return 1;
  if (resize ? launch_preprocess_rgb_resize(df, dtype, B, Hs, Ws, Hr, Wr, pad_t, pad_l, Hp, Wp, dout, nullptr)
             : launch_preprocess_rgb(df, dtype, B, Hs, Ws, pad_t, pad_l, Hp, Wp, dout, nullptr)) return 1;
  if (g.check("odt_op_preprocess_rgb")) return 1;
  return get_dev(out, dout, (size_t)B * Hp * Wp * 4);
}

int odt_op_mask_rle(int device, const float* masks, const float* boxes, int n, int on_device, int height, int width,
                    double scale, int want_counts, odt_rle_result* out) {
  ODT_CHECK(out != nullptr && (n == 0 || (masks && boxes)), "odt_op_mask_rle: null argument");
  ODT_CHECK(n >= 0, "odt_op_mask_rle: bad number of detections");
  if (set_dev(device)) return 1;
  static thread_local MaskRleHost res;      // (the result stays readable until this thread's next call)
  GBufs g;
  MaskRleParams p; std::memset(&p, 0, sizeof(p));
  p.masks = masks; p.boxes = boxes;
  if (!on_device && n > 0) {
    float *dm, *db;
    if (g.alloc("masks", (size_t)n * 784, &dm, -1, masks) || g.alloc("boxes", (size_t)n * 4, &db, -1, boxes)) return 1;
    p.masks = dm; p.boxes = db;
  }
  p.R = n; p.n = n; p.H0 = height; p.W0 = width; p.scale = (float)scale;
  auto alloc = [&g](const char* name, size_t bytes, void** dev) -> int {
    unsigned char* d;
    if (g.alloc(name, bytes, &d)) return 1;
    *dev = d;
    return 0;
  };
  if (run_mask_rle(p, want_counts != 0, nullptr, alloc, res) || g.check("odt_op_mask_rle")) return 1;
  rle_fill(res, out);
  return 0;
}

}  // extern "C"
