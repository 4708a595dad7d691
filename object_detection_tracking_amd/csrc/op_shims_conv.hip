// The stand-alone conv entry points of the C ABI (include/odt.h: odt_op_conv2d, odt_op_conv2d_cat, odt_op_bottleneck_tail,
// odt_op_bottleneck_block, odt_op_stem, odt_op_conv_choice, odt_op_last_conv) and the record helpers they share with
// odt_op_se_tail (op_shims.hip).  The fusion shims turn their records into the fused ones with the functions the plan's fuse_*
// passes call (conv_h2f_fuse, conv_block_fuse, conv_stem_fuse: odt_common.hpp), so a test of a shim tests the plan's rewrite.
#include "op_shims.hpp"

namespace odt {

namespace {

// what the stand-alone conv entry points launched last on this thread (odt_op_last_conv): the finished record's row and
// launch choices, kept at the launch points below.  Host only; nothing on the plan's path writes or reads it.
struct LastConv { int variant = CV_NONE, splitk = 0, reduce_blocks = 0; };
thread_local LastConv g_last_conv;

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

// this record runs row `variant` on the fp16x2 kernels: its sources' and its output's range slots, the derived fields, its
// weight image
int use_h2_row(GBufs& g, ConvParams& p, int variant, const unsigned* in_amax, unsigned* out_amax) {
  conv_use_variant(p, variant);
  p.in_amax = in_amax; p.out_amax = out_amax;
  conv_prepare(p);
  float* img;
  if (g.alloc("weight image", (conv_split_weight_bytes(p.Cout, conv_k(p)) + 3) / 4, &img) || conv_make_split_weights(p, img, nullptr)) return 1;
  conv_attach_weights(p, img);
  return 0;
}

// conv2 (3x3, stride 1, 'SAME' for dilation dil, C -> C, bias, ReLU: in -> mid, a sentinel-filled [M,C] tensor of g) and conv3
// (1x1, C -> C3, bias (+ res), ReLU?: mid -> out) of a bottleneck from the caller's host weights, as prepared fp16x2 records;
// slot: three range slots in a row, of in, mid and out.  fuse: the pair as conv_h2f_fuse rewrites it (a carries the tail, b
// stays its partner record)
struct ConvPair { ConvParams a, b; };
int bottleneck_pair(GBufs& g, const char* op, const float* in, float* out, const float* w2_hwio, const float* b2, const float* w3_io,
                    const float* b3, const float* res, int B, int H, int W, int C, int dil, int C3, int relu3, unsigned* slot, int fuse,
                    ConvPair* pr) {
  const std::vector<float> w2 = ohwi(w2_hwio, 3, 3, C, C), w3 = ohwi(w3_io, 1, 1, C, C3);
  float *dw2, *db2, *dw3, *db3, *mid;
  if (g.alloc("w2", w2.size(), &dw2, -1, w2.data()) || g.alloc("b2", (size_t)C, &db2, -1, b2) || g.alloc("w3", w3.size(), &dw3, -1, w3.data()) ||
      g.alloc("b3", (size_t)C3, &db3, -1, b3) || g.alloc("conv2 out", (size_t)B * H * W * C, &mid)) return 1;
  ConvParams& a = pr->a;
  ConvParams& b = pr->b;
  a = same_conv(in, dw2, db2, mid, B, H, W, C, C, 3, dil, 1);
  a.debug = 0x400;
  if (use_h2_row(g, a, conv_variant_find(CF_H2, 256, C, CVF_KWR), slot, slot + kAmaxWays)) return 1;
  b = same_conv(mid, dw3, db3, out, B, H, W, C, C3, 1, 1, relu3 ? 1 : 0);
  b.res = res; b.res_mode = res ? 1 : 0; b.res_H = H; b.res_W = W; b.res_ldc = C3; b.debug = 0x400;
  if (use_h2_row(g, b, C3 % 256 == 0 ? CV_H2_256x256 : (C3 % 128 == 0 ? CV_H2_256x128 : CV_H2_128x64), slot + kAmaxWays, slot + 2 * kAmaxWays)) return 1;
  if (fuse) {
    ODT_CHECK(conv_h2f_fusable(a, b), std::string(op) + ": conv2 + conv3 are not fusable");
    float* imgf;
    if (g.alloc("fused tail weights", (conv_h2f_weight_bytes(C3, C) + 3) / 4, &imgf) || conv_make_h2f_weights(dw3, C3, C, imgf, nullptr)) return 1;
    conv_h2f_fuse(a, b, imgf);
  }
  return 0;
}

// the end of a fusion shim: check the first nlaunch records, upload all of them in this order (a fused record's partners
// travel with it although only it is launched), note the last launched one, launch in order on the null stream
int launch_records(GBufs& g, const std::vector<ConvParams>& recs, size_t nlaunch,
                   int (*launch)(const ConvParams&, const ConvParams*, hipStream_t) = launch_conv) {
  for (size_t i = 0; i < nlaunch; ++i) if (conv_check(recs[i])) return 1;
  ConvParams* dev;
  if (g.alloc("conv records", recs.size(), &dev, -1, recs.data())) return 1;
  note_conv(recs[nlaunch - 1]);
  for (size_t i = 0; i < nlaunch; ++i) if (launch(recs[i], dev + i, nullptr)) return 1;
  return 0;
}

// ODT_CONV_TRACE reports (tuning aids; at the end of this file)
int report_conv_trace(const unsigned long long* tr, int max_blocks);
int report_block_trace(const unsigned long long* tr, size_t ntile);

}  // namespace

void note_conv(const ConvParams& q) { g_last_conv.variant = q.variant; g_last_conv.splitk = q.splitk; g_last_conv.reduce_blocks = q.reduce_blocks; }

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

// one stand-alone conv (odt_op_conv2d*, odt_op_se_tail: dense tensors, null stream) as a plan would run it: the library's
// policy under the call's knobs, a weight image / split-K scratch / input range in g where the split kernels take them, a
// finished record.  Returns with the launch in flight: g waits for it (check, or its destructor).
int run_conv(GBufs& g, ConvParams q, const Knobs& kn) {
  if (conv_check(q)) return 1;
  conv_prepare(q);
  const ConvPolicy pol = conv_policy_with_knobs(conv_policy_default(), kn);
  ConvChoice ch = conv_select(q, pol, kn);
  if (conv_variant_row(ch.variant).family != CF_F32) {
    unsigned char* img;
    if (g.alloc("weight image", conv_split_weight_bytes(q.Cout, conv_k(q)), &img)) return 1;
    if (pol.family == 2 && q.in_amax == nullptr) {      // fp16x2 pieces need the sources' |max|: nobody recorded it for a stand-alone call
      // (the scan covers the whole allocation B x in_Ha x in_Wa x in_ldc of a source: a stand-alone caller hands over
      // dense tensors -- odt_op_conv2d* -- so this is the logical view; a sliced view would have to bring its own range)
      unsigned* amax;
      if (alloc_amax(g, &amax, 2) || launch_tensor_amax(q.in, (size_t)q.B * q.in_Ha * q.in_Wa * q.in_ldc, amax, nullptr)) return 1;
      q.in_amax = amax;
      if (q.in2 != nullptr) {
        if (launch_tensor_amax(q.in2, (size_t)q.B * q.in2_Ha * q.in2_Wa * q.in2_ldc, amax + kAmaxWays, nullptr)) return 1;
        q.in2_amax = amax + kAmaxWays;
      }
      ch = conv_select(q, pol, kn);       // (with the ranges: whether a layer takes the split kernels does not depend on them, which ones does)
    }
    conv_use_variant(q, ch.variant, ch.splitk, ch.reduce_blocks);
    if (conv_make_split_weights(q, img, nullptr)) return 1;
    conv_attach_weights(q, img);
    if (conv_split_partial_bytes(q) > 0 && g.alloc("split-K partial sums", conv_split_partial_bytes(q) / sizeof(float), &q.partial)) return 1;
  }
  if (conv_finish(q, kn)) return 1;
  note_conv(q);
  ConvParams* rec;
  if (g.alloc("conv record", 1, &rec, -1, &q)) return 1;
  return launch_conv(q, rec, nullptr);
}

}  // namespace odt

using namespace odt;

extern "C" {

int odt_op_conv2d(int device, const float* in, int B, int H, int W, int Cin, const float* wt_hwio,
                  const float* bias, int kh, int kw, int Cout, int stride, int dil, int pad_t, int pad_l,
                  int Ho, int Wo, int oy, int ox, const float* res, int res_mode, int relu, float* out) {
  ODT_CHECK(in && wt_hwio && out, "odt_op_conv2d: null argument");
  if (set_dev(device)) return 1;
  const size_t nin = (size_t)B * H * W * Cin, nout = (size_t)B * (Ho + oy) * (Wo + ox) * Cout;
  const std::vector<float> w = ohwi(wt_hwio, kh, kw, Cin, Cout), bz(Cout, 0.f);
  const int rH = res_mode == 2 ? (Ho + 1) / 2 : Ho, rW = res_mode == 2 ? (Wo + 1) / 2 : Wo;
  GBufs g;
  float *di, *dw, *db, *dr = nullptr, *dout;
  if (g.alloc("in", nin, &di, -1, in) || g.alloc("wt", w.size(), &dw, -1, w.data()) ||
      g.alloc("bias", (size_t)Cout, &db, -1, bias ? bias : bz.data()) || g.alloc("out", nout, &dout, 0)) return 1;
  if (res && res_mode && g.alloc("res", (size_t)B * rH * rW * Cout, &dr, -1, res)) return 1;
  ConvParams p = dense_conv(di, dw, db, dout, B, H, W, Cin, Ho, Wo, Cout, kh, kw, stride, dil, pad_t, pad_l, relu);
  p.out_H = Ho + oy; p.out_W = Wo + ox; p.out_oy = oy; p.out_ox = ox;
  p.res = dr; p.res_mode = dr ? res_mode : 0; p.res_H = rH; p.res_W = rW; p.res_ldc = Cout;
  const Knobs kn = knobs_read();      // (the environment as it is at this call)
  const bool trace = kn.get(K_CONV_TRACE).set;
  const size_t ntrace = (size_t)(1 << 16) * 16;
  if (trace && g.alloc("trace", ntrace, &p.trace, 0)) return 1;
  if (run_conv(g, p, kn)) return 1;      // warm
  if (trace) ODT_HIP(hipMemset(p.trace, 0, ntrace * sizeof(*p.trace)));
  if (run_conv(g, p, kn)) return 1;
  if (g.check("odt_op_conv2d")) return 1;
  if (trace && report_conv_trace(p.trace, 1 << 16)) return 1;
  return get_dev(out, dout, nout);
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
  GBufs g;
  float *da, *db2, *dw, *dbias, *dout;
  const size_t na = (size_t)B * Ho * Wo * Ca, nb = (size_t)B * Hb * Wb * Cb, nout = (size_t)B * Ho * Wo * Cout;
  if (g.alloc("a", na, &da, -1, a) || g.alloc("b", nb, &db2, -1, b2) || g.alloc("wt", w.size(), &dw, -1, w.data()) ||
      g.alloc("bias", (size_t)Cout, &dbias, -1, bias ? bias : bz.data()) || g.alloc("out", nout, &dout, 0)) return 1;
  ConvParams p = same_conv(da, dw, dbias, dout, B, Ho, Wo, Ca, Cout, 1, 1, relu);
  p.in2 = db2; p.Cin2 = Cb; p.in2_ldc = Cb; p.in2_Ha = Hb; p.in2_Wa = Wb; p.in2_stride = stride_b;
  if (run_conv(g, p, knobs_read()) || g.check("odt_op_conv2d_cat")) return 1;
  return get_dev(out, dout, nout);
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
  GBufs g;
  float *di, *dres = nullptr, *dout;
  unsigned* amax;      // ranges of in, conv2's and conv3's output
  if (g.alloc("in", M * C, &di, -1, in) || g.alloc("out", M * C3, &dout, 0) || alloc_amax(g, &amax, 4)) return 1;
  if (res && g.alloc("res", M * C3, &dres, -1, res)) return 1;
  if (launch_tensor_amax(di, M * C, amax, nullptr)) return 1;
  ConvPair pr;
  if (bottleneck_pair(g, "odt_op_bottleneck_tail", di, dout, w2_hwio, b2, w3_io, b3, dres, B, H, W, C, dil, C3, relu3, amax, fuse, &pr)) return 1;
  if (launch_records(g, {pr.a, pr.b}, fuse ? 1 : 2) || g.check("odt_op_bottleneck_tail")) return 1;
  return get_dev(out, dout, M * C3);
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
  const std::vector<float> w1 = ohwi(w1_io, 1, 1, C4, C);
  GBufs g;
  float *dx, *dw1, *db1, *dt1, *dout;
  unsigned* amax;      // ranges of x, t1, t2, out
  if (g.alloc("x", M * C4, &dx, -1, x) || g.alloc("w1", w1.size(), &dw1, -1, w1.data()) || g.alloc("b1", (size_t)C, &db1, -1, b1) ||
      g.alloc("t1", M * C, &dt1) || g.alloc("out", M * C4, &dout, 0) || alloc_amax(g, &amax, 4)) return 1;
  if (launch_tensor_amax(dx, M * C4, amax, nullptr)) return 1;
  ConvParams c1 = same_conv(dx, dw1, db1, dt1, B, H, W, C4, C, 1, 1, 1);
  if (use_h2_row(g, c1, CV_H2_128x64, amax, amax + kAmaxWays)) return 1;
  ConvPair pr;
  if (bottleneck_pair(g, "odt_op_bottleneck_block", dt1, dout, w2_hwio, b2, w3_io, b3, dx, B, H, W, C, 1, C4, 1, amax + kAmaxWays, fuse, &pr)) return 1;
  if (fuse) {
    ODT_CHECK(conv_block_fits(c1, pr.a), "odt_op_bottleneck_block: this block does not fit conv_block_kernel");
    float* img2p;
    if (g.alloc("conv2 patch weights", (conv_split_weight_bytes(C, 9 * C) + 3) / 4, &img2p) || conv_make_h2p_weights(pr.a, img2p, nullptr)) return 1;
    conv_block_fuse(pr.a, c1, img2p);      // (t1 does not exist)
    // ODT_CONV_TRACE (tuning): per-phase wall-clock (100 MHz) averages over the workgroups
    const bool trace = knobs_read().get(K_CONV_TRACE).set;
    const size_t ntile = (size_t)B * ((H + 15) / 16) * ((W + 15) / 16);
    if (trace && g.alloc("trace", ntile * 16, &pr.a.trace, 0)) return 1;
    if (launch_records(g, {pr.a, c1, pr.b}, 1, launch_bottleneck_block)) return 1;
    if (trace && report_block_trace(pr.a.trace, ntile)) return 1;
  } else if (launch_records(g, {c1, pr.a, pr.b}, 3)) {
    return 1;
  }
  if (g.check("odt_op_bottleneck_block")) return 1;
  return get_dev(out, dout, M * C4);
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
  GBufs g;
  float *di, *dw, *db, *dmap, *dout;
  unsigned* amax;
  const size_t nmap = (size_t)B * Ho0 * Wo0 * 64, nout = (size_t)B * Hq * Wq * 64;
  if (g.alloc("frames", x.size(), &di, -1, x.data()) || g.alloc("wt", wv.size(), &dw, -1, wv.data()) || g.alloc("bias", (size_t)64, &db, -1, bias) ||
      g.alloc("conv0 map", nmap, &dmap) || g.alloc("out", nout, &dout, 0) || alloc_amax(g, &amax, 4)) return 1;
  if (launch_tensor_amax(di, x.size(), amax, nullptr)) return 1;
  ConvParams p = dense_conv(di, dw, db, dmap, B, Hp, Wa, 32, Ho0, Wo0, 64, 7, 1, 2, 1, 0, 0, 1);
  p.in_ldc = 4;      // (Cin = 32: eight 4-channel pixels)
  if (use_h2_row(g, p, CV_H2_128x64, amax, amax + kAmaxWays)) return 1;
  if (fuse) {
    ODT_CHECK(conv_stem_fits(p), "odt_op_stem: shape not taken by the stem kernel");
    conv_stem_fuse(p, dout, Hq, Wq, p.out_ldc);
    if (grid > 0) p.debug |= (grid & 0x3ff) << 20;
  }
  if (launch_records(g, {p}, 1)) return 1;
  if (!fuse && launch_maxpool3x3s2(dmap, B, Ho0, Wo0, 64, dout, Hq, Wq, nullptr)) return 1;
  if (g.check("odt_op_stem")) return 1;
  return get_dev(out, dout, nout);
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

}  // extern "C"

namespace odt {
namespace {

// ODT_CONV_TRACE report of odt_op_conv2d (tuning aid): per-phase wall-clock (100 MHz) statistics over the workgroups
int report_conv_trace(const unsigned long long* tr, int max_blocks) {
  std::vector<unsigned long long> t((size_t)max_blocks * 16);
  if (get_dev(t.data(), tr, t.size())) return 1;
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
int report_block_trace(const unsigned long long* tr, size_t ntile) {
  ODT_HIP(hipDeviceSynchronize());
  std::vector<unsigned long long> t(ntile * 16);
  if (get_dev(t.data(), tr, t.size())) return 1;
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

}  // namespace
}  // namespace odt
