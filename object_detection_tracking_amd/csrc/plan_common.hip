// Plan-building helpers shared by the FPN detector plan (plan_fpn.hip) and the EfficientDet plan (plan_effdet.hip):
// tensors (dedicated or arena-planned), weight upload with BN folding, conv ops, bf16x3 weight images, the RPN-head
// fusion and the activation arena.
#include "odt_model.hpp"

#define g_err (::odt::last_error())

namespace odt {

int ceil_div(int a, int b) { return (a + b - 1) / b; }

int make_tensor(odt_model* m, const std::string& name, int B, int H, int W, int C, Tensor* t, bool zero) {
  t->B = B; t->H = H; t->W = W; t->C = C; t->h = H; t->w = W; t->c = C;
  if (m->arena_on && !zero) {
    // (zero == true means "regions the kernels never write must read as zero": such a tensor cannot share memory)
    odt_model::VTensor v;
    v.bytes = (t->elems() * sizeof(float) + 255) & ~(size_t)255;
    v.voff = m->vnext;
    m->vnext += v.bytes;
    m->vt.push_back(v);
    m->virtual_tensor_bytes += v.bytes;
    t->d = reinterpret_cast<float*>(odt_model::kVirtBase + v.voff);
    if (!name.empty()) m->taps[name] = *t;
    return 0;
  }
  t->d = m->alloc_f(t->elems(), zero);
  ODT_CHECK(t->d != nullptr, "device allocation failed for " + name + ": " + g_err);
  m->dedicated_tensor_bytes += t->elems() * sizeof(float);
  if (!name.empty()) m->taps[name] = *t;
  return 0;
}

const HostTensor* find_w(odt_model* m, const std::string& name) {
  auto it = m->host_w.find(name);
  return it == m->host_w.end() ? nullptr : &it->second;
}

// TensorFlow's 'SAME' geometry (conv2d's default padding, nn.py:337-381): out = ceil(in / s), the smaller half of the padding
// in front.  The rest lies behind the input, where the kernels read zeros anyway.  Returns the padding of both sides together.
int same_pad(int in, int k, int s, int* out, int* before) {
  *out = (in + s - 1) / s;
  const int tot = std::max((*out - 1) * s + k - in, 0);
  *before = tot / 2;
  return tot;
}

// BN fold factors of the c channels of `scope`, in double: tf.nn.batch_normalization (nn.py:1771-1774).  The detector's
// variables are bn/gamma, bn/beta, bn/mean/EMA, bn/variance/EMA (eps 1e-5); a Keras BatchNormalization scope (keras) holds
// gamma, beta, moving_mean, moving_variance (EfficientDet: eps 1e-3).
int bn_fold(odt_model* m, const std::string& scope, int c, double eps, bool keras, std::vector<double>* scale,
            std::vector<double>* shift) {
  const HostTensor* g = find_w(m, scope + (keras ? "/gamma" : "/bn/gamma"));
  const HostTensor* b = find_w(m, scope + (keras ? "/beta" : "/bn/beta"));
  const HostTensor* mu = find_w(m, scope + (keras ? "/moving_mean" : "/bn/mean/EMA"));
  const HostTensor* var = find_w(m, scope + (keras ? "/moving_variance" : "/bn/variance/EMA"));
  ODT_CHECK(g && b && mu && var, "missing BN variables for " + scope);
  ODT_CHECK(g->data.size() == (size_t)c && b->data.size() == (size_t)c && mu->data.size() == (size_t)c &&
            var->data.size() == (size_t)c, "bad BN shapes for " + scope);
  scale->resize(c); shift->resize(c);
  for (int o = 0; o < c; ++o) {
    const double inv = (double)g->data[o] / std::sqrt((double)var->data[o] + eps);
    (*scale)[o] = inv;
    (*shift)[o] = (double)b->data[o] - (double)mu->data[o] * inv;
  }
  return 0;
}

static int upload_conv_scaled(odt_model* m, const HostTensor& Wt, int kh, int kw, int cin, int cout, const std::vector<double>& scale,
                              const std::vector<double>& shift, const float** wt_out, const float** bias_out);

// Upload conv weights in [Cout][kh][kw][Cin] with optional folded BN; returns device ptrs.
int upload_conv(odt_model* m, const std::string& scope, int kh, int kw, int cin, int cout,
                bool has_bn, const float** wt_out, const float** bias_out) {
  const HostTensor* W = find_w(m, scope + "/W");
  ODT_CHECK(W != nullptr, "missing weight " + scope + "/W");
  ODT_CHECK(W->data.size() == (size_t)kh * kw * cin * cout,
            "bad shape for " + scope + "/W");
  std::vector<double> scale(cout, 1.0), shift(cout, 0.0);
  if (has_bn) {
    if (bn_fold(m, scope, cout, 1e-5, false, &scale, &shift)) return 1;
  } else {
    const HostTensor* b = find_w(m, scope + "/b");
    ODT_CHECK(b != nullptr, "missing bias " + scope + "/b");
    for (int o = 0; o < cout; ++o) shift[o] = b->data[o];
  }
  return upload_conv_scaled(m, *W, kh, kw, cin, cout, scale, shift, wt_out, bias_out);
}

// A conv that GroupNorm follows (odt_config.use_gn): the weights as they are -- nothing can be folded, the statistics come from
// the frame -- with the layer's own bias (the FPN convs) or a zero one (the backbone convs have none).
int upload_conv_plain(odt_model* m, const std::string& scope, int kh, int kw, int cin, int cout, bool has_bias, const float** wt_out,
                      const float** bias_out) {
  const HostTensor* W = find_w(m, scope + "/W");
  ODT_CHECK(W != nullptr, "missing weight " + scope + "/W");
  ODT_CHECK(W->data.size() == (size_t)kh * kw * cin * cout, "bad shape for " + scope + "/W");
  std::vector<double> scale(cout, 1.0), shift(cout, 0.0);
  if (has_bias) {
    const HostTensor* b = find_w(m, scope + "/b");
    ODT_CHECK(b != nullptr, "missing bias " + scope + "/b");
    ODT_CHECK(b->data.size() == (size_t)cout, "bad shape for " + scope + "/b");
    for (int o = 0; o < cout; ++o) shift[o] = b->data[o];
  }
  return upload_conv_scaled(m, *W, kh, kw, cin, cout, scale, shift, wt_out, bias_out);
}

// HWIO weights times scale[o] -> [Cout][kh][kw][Cin] and shift -> bias, on the device
static int upload_conv_scaled(odt_model* m, const HostTensor& Wt, int kh, int kw, int cin, int cout, const std::vector<double>& scale,
                       const std::vector<double>& shift, const float** wt_out, const float** bias_out) {
  const HostTensor* W = &Wt;
  std::vector<float> wt((size_t)cout * kh * kw * cin), bias(cout);
  for (int y = 0; y < kh; ++y)
    for (int x = 0; x < kw; ++x)
      for (int i = 0; i < cin; ++i)
        for (int o = 0; o < cout; ++o)
          wt[(((size_t)o * kh + y) * kw + x) * cin + i] =
              (float)((double)W->data[(((size_t)y * kw + x) * cin + i) * cout + o] * scale[o]);
  for (int o = 0; o < cout; ++o) bias[o] = (float)shift[o];
  return upload_raw(m, wt, wt_out) || upload_raw(m, bias, bias_out);
}

// conv3 + convshortcut of a stage-entry bottleneck as ONE 1x1 conv over the K-concatenated input
// [t2 | x]: weights [cout][cin_a + cin_b] with each part's BN folded in, bias = shift_a + shift_b
// (reference nn.py:503-521: conv3 -> BN, shortcut conv -> BN, add, ReLU).
int upload_conv_cat(odt_model* m, const std::string& sa, int cin_a, const std::string& sb, int cin_b, int cout,
                    const float** wt_out, const float** bias_out) {
  std::vector<float> wt((size_t)cout * (cin_a + cin_b));
  std::vector<double> shift(cout, 0.0), inv, sh;
  const std::string scopes[2] = {sa, sb};
  const int cins[2] = {cin_a, cin_b};
  int koff = 0;
  for (int part = 0; part < 2; ++part) {
    const std::string& scope = scopes[part];
    const int cin = cins[part];
    const HostTensor* W = find_w(m, scope + "/W");
    ODT_CHECK(W != nullptr, "missing weight " + scope + "/W");
    ODT_CHECK(W->data.size() == (size_t)cin * cout, "bad shape for " + scope + "/W");
    if (bn_fold(m, scope, cout, 1e-5, false, &inv, &sh)) return 1;
    for (int o = 0; o < cout; ++o) {
      shift[o] += sh[o];
      for (int i = 0; i < cin; ++i)
        wt[(size_t)o * (cin_a + cin_b) + koff + i] = (float)((double)W->data[(size_t)i * cout + o] * inv[o]);
    }
    koff += cin;
  }
  std::vector<float> bias(cout);
  for (int o = 0; o < cout; ++o) bias[o] = (float)shift[o];
  return upload_raw(m, wt, wt_out) || upload_raw(m, bias, bias_out);
}

// The ResNeXt block's grouped conv2 (W [3,3,C/32,C], nn.py:536-539) with its BN folded in double, as upload_conv does, and
// re-packed for the kernel (group_conv_pack_weights).
int upload_group_conv(odt_model* m, const std::string& scope, int C, const float** wt_out, const float** bias_out) {
  const HostTensor* W = find_w(m, scope + "/W");
  ODT_CHECK(W != nullptr, "missing weight " + scope + "/W");
  ODT_CHECK(W->data.size() == group_conv_weight_elems(C), "bad shape for " + scope + "/W (a 32-group 3x3 conv: [3,3,C/32,C])");
  std::vector<double> scale, shift;
  if (bn_fold(m, scope, C, 1e-5, false, &scale, &shift)) return 1;
  std::vector<float> bias(C), img(group_conv_weight_elems(C));
  for (int o = 0; o < C; ++o) bias[o] = (float)shift[o];
  if (group_conv_pack_weights(W->data.data(), scale.data(), C, img.data())) return 1;
  return upload_raw(m, img, wt_out) || upload_raw(m, bias, bias_out);
}

// A deformable stage entry's conv2_offset (W [3,3,C,18] + b [18]: a bias, no BN) and conv2 (W [3,3,C,C]: neither bias nor BN,
// nn.py:474-485 -- nothing is folded), re-packed for the kernels (conv_deform.hip).
int upload_deform_conv(odt_model* m, const std::string& pre, int C, const float** wt_off, const float** b_off, const float** wt) {
  const HostTensor* Wo = find_w(m, pre + "/conv2_offset/W");
  const HostTensor* bo = find_w(m, pre + "/conv2_offset/b");
  const HostTensor* W = find_w(m, pre + "/conv2/W");
  ODT_CHECK(Wo != nullptr && bo != nullptr, "missing weight " + pre + "/conv2_offset/{W,b} (a deformable block: odt_config.use_deformable)");
  ODT_CHECK(W != nullptr, "missing weight " + pre + "/conv2/W");
  ODT_CHECK(Wo->data.size() == (size_t)9 * C * 18 && bo->data.size() == 18, "bad shape for " + pre + "/conv2_offset (W [3,3,C,18], b [18])");
  ODT_CHECK(W->data.size() == (size_t)9 * C * C, "bad shape for " + pre + "/conv2/W");
  std::vector<float> io(deform_offset_weight_elems(C)), iw(deform_weight_elems(C));
  if (deform_pack_offset_weights(Wo->data.data(), C, io.data()) || deform_pack_weights(W->data.data(), C, iw.data())) return 1;
  return upload_raw(m, io, wt_off) || upload_raw(m, bo->data, b_off) || upload_raw(m, iw, wt);
}

// The SE gate of bottleneck `pre` (reference nn.py:506-517) with conv3 + BN folded into fc1.  conv3 is 1x1 and BN affine, so
// mean_HW(BN(conv3(t2))) = BN(conv3(mean_HW(t2))):
//   w1[j][i] = sum_o conv3/W[i][o] * bnscale[o] * fc1/W[o][j]      b1[j] = sum_o bnshift[o] * fc1/W[o][j] + fc1/b[j]
// in double, rounded to f32 once; w2t = fc2/W as it is ([in, out] = [r][4 ch]).
int upload_se_gate(odt_model* m, const std::string& pre, int ch, const float** w1, const float** b1, const float** w2t,
                   const float** b2) {
  const int C4 = ch * 4, r = ch / 4;
  const HostTensor* W3 = find_w(m, pre + "/conv3/W");
  const HostTensor* f1 = find_w(m, pre + "/fc1/W");
  const HostTensor* f1b = find_w(m, pre + "/fc1/b");
  const HostTensor* f2 = find_w(m, pre + "/fc2/W");
  const HostTensor* f2b = find_w(m, pre + "/fc2/b");
  ODT_CHECK(W3 != nullptr, "missing conv3 variables for the SE gate of " + pre);
  ODT_CHECK(f1 && f1b && f2 && f2b, "missing squeeze-excitation variables " + pre + "/fc1, fc2");
  ODT_CHECK(W3->data.size() == (size_t)ch * C4, "bad conv3 shapes for the SE gate of " + pre);
  ODT_CHECK(f1->data.size() == (size_t)C4 * r && f1b->data.size() == (size_t)r && f2->data.size() == (size_t)r * C4 &&
            f2b->data.size() == (size_t)C4, "bad squeeze-excitation shapes in " + pre);
  std::vector<double> scale, shift, acc(r);
  if (bn_fold(m, pre + "/conv3", C4, 1e-5, false, &scale, &shift)) return 1;
  std::vector<float> v1((size_t)r * ch), vb(r);
  for (int j = 0; j < r; ++j) acc[j] = (double)f1b->data[j];
  for (int o = 0; o < C4; ++o)
    for (int j = 0; j < r; ++j) acc[j] += shift[o] * (double)f1->data[(size_t)o * r + j];
  for (int j = 0; j < r; ++j) vb[j] = (float)acc[j];
  for (int i = 0; i < ch; ++i) {
    std::fill(acc.begin(), acc.end(), 0.0);
    for (int o = 0; o < C4; ++o) {
      const double a = (double)W3->data[(size_t)i * C4 + o] * scale[o];
      const float* f = &f1->data[(size_t)o * r];
      for (int j = 0; j < r; ++j) acc[j] += a * (double)f[j];
    }
    for (int j = 0; j < r; ++j) v1[(size_t)j * ch + i] = (float)acc[j];
  }
  return upload_raw(m, v1, w1) || upload_raw(m, vb, b1) || upload_raw(m, f2->data, w2t) || upload_raw(m, f2b->data, b2);
}

int upload_raw(odt_model* m, const std::vector<float>& v, const float** out) {
  float* d = m->alloc_f(v.size(), false);
  ODT_CHECK(d != nullptr, "device allocation failed");
  ODT_HIP(hipMemcpy(d, v.data(), v.size() * sizeof(float), hipMemcpyHostToDevice));
  *out = d;
  return 0;
}

// Append the conv op of `s`.  The output tensor is created here unless `out` already holds one.
int add_conv(odt_model* m, const ConvSpec& s, Tensor* out) {
  ConvOp c;
  c.name = s.name;
  ConvParams& p = c.p;
  std::memset(&p, 0, sizeof(p));
  const Tensor& in = s.in;
  const int Ho = s.Ho >= 0 ? s.Ho : in.h, Wo = s.Wo >= 0 ? s.Wo : in.w;
  const int out_ldc = s.out_ldc >= 0 ? s.out_ldc : s.cout;
  if (out->d == nullptr) {
    if (make_tensor(m, s.tap, in.B, Ho + s.oy, Wo + s.ox, out_ldc, out, s.oy != 0 || s.ox != 0 || out_ldc != s.cout))
      return 1;
    out->c = s.cout;
  }
  p.in = in.d; p.wt = s.wt; p.bias = s.bias; p.out = out->d;
  p.res = s.res ? s.res->d : nullptr;
  p.B = in.B; p.H = in.h; p.W = in.w; p.Cin = s.cin; p.in_ldc = in.C;
  p.in_Ha = in.H; p.in_Wa = in.W;   // sliced views keep the allocation pitch
  p.Ho = Ho; p.Wo = Wo; p.Cout = s.cout;
  p.kh = s.kh; p.kw = s.kw; p.stride = s.stride; p.dil = s.dil; p.pad_t = s.pad_t; p.pad_l = s.pad_l;
  p.out_H = out->H; p.out_W = out->W; p.out_oy = s.oy; p.out_ox = s.ox; p.out_ldc = out->C;
  p.res_mode = s.res ? s.res_mode : 0;
  if (s.res) { p.res_H = s.res->H; p.res_W = s.res->W; p.res_ldc = s.res->C; }
  p.relu = s.relu;
  if (s.in2) {
    p.in2 = s.in2->d; p.Cin2 = s.cin2; p.in2_ldc = s.in2->C; p.in2_Ha = s.in2->H; p.in2_Wa = s.in2->W; p.in2_stride = s.in2_stride;
  }
  conv_prepare(p);
  m->convs.push_back(c);
  Op op;
  op.kind = OP_CONV;
  op.conv = (int)m->convs.size() - 1;
  m->ops.push_back(op);
  return 0;
}

// A handle's side streams (tail, H2D, D2H) are created with the highest stream priority.  Not for the arbitration: the
// runtime multiplexes all streams of ONE priority onto a few hardware queues in creation order, and a side stream that
// lands on the main stream's queue is serialised behind the forward it is meant to overlap (seen with the tracker's
// stream: tools/experiments/track_stream_collision.py); streams of another priority get queues of their own.
// ODT_SIDE_STREAM_PRIORITY=0: plain streams (A/B).
int create_side_stream(hipStream_t* s, const Knobs& k) {
  const bool flat = k.off(K_SIDE_STREAM_PRIORITY);
  if (flat) { ODT_HIP(hipStreamCreateWithFlags(s, hipStreamNonBlocking)); return 0; }
  int least = 0, greatest = 0;
  ODT_HIP(hipDeviceGetStreamPriorityRange(&least, &greatest));
  ODT_HIP(hipStreamCreateWithPriority(s, hipStreamNonBlocking, greatest));
  return 0;
}

// bf16-piece weight images (conv_split.hip) for the plan's convs that the split kernel takes
// the handle's conv policy: odt_config first, ODT_CONV_* debug overrides on top
ConvPolicy resolve_conv_policy(const odt_model* m) {
  ConvPolicy pol = conv_policy_default();
  if (m->cfg.conv_arith == ODT_ARITH_F32) pol.arith = 0;
  else if (m->cfg.conv_arith == ODT_ARITH_BF16X3) pol.arith = 1;
  if (m->cfg.conv_split_family >= 1 && m->cfg.conv_split_family <= 3) pol.family = m->cfg.conv_split_family;
  pol = conv_policy_with_knobs(pol, m->knobs);
  // (the EfficientDet graph keeps the bf16x3 kernels: its convs mostly lack 256-row x 128-column tiles, and its in-place
  // gates would need their own range bookkeeping)
  if (m->cfg.graph == ODT_GRAPH_EFFNET && pol.family == 2) pol.family = 3;
  return pol;
}

int attach_split_weights(odt_model* m) {
  const ConvPolicy pol = resolve_conv_policy(m);
  m->policy = pol;
  if (pol.arith == 0) return 0;
  find_overlap_points(m);
  // [live |max|][previous forward's |max|], kRangeSlots words each (odt_common.hpp)
  static_assert(2 * odt_model::kAmaxSlots * kAmaxWays == kRangeSlots, "the range records are laid out for one word per slot");
  m->amax_dev = reinterpret_cast<unsigned*>(m->alloc_f((size_t)2 * kRangeSlots, true));
  ODT_CHECK(m->amax_dev != nullptr, "device allocation failed (range slots)");
  if (m->range_host == nullptr) {
    // what the previous forward recorded, where the host can read it without a copy or a synchronisation (odt_range_health)
    ODT_HIP(hipHostMalloc((void**)&m->range_host, (size_t)kRangeSlots * sizeof(unsigned), hipHostMallocMapped));
    std::memset(m->range_host, 0, (size_t)kRangeSlots * sizeof(unsigned));
    ODT_HIP(hipHostGetDevicePointer((void**)&m->range_host_dev, m->range_host, 0));
  }
  m->range_slot_name.assign(kRangeSlots, std::string());
  m->range_baseline.assign(kRangeSlots, 0.f);
  // |max| slots: a tensor written by a split conv kernel gets one; a pooled / subsampled tensor shares its source's (its
  // values are a subset); anything else has none, and a conv reading it stays off the fp16x2 kernels.  Tail convs only
  // see slots filled in the tail (the trunk group is cleared by the next forward while the tail may still be running).
  std::map<const float*, int> slot_of;
  auto slot_ptr = [&](const float* t, bool tail_reader) -> const unsigned* {
    auto it = t != nullptr ? slot_of.find(t) : slot_of.end();
    if (it == slot_of.end()) return nullptr;
    if (tail_reader != (it->second >= odt_model::kAmaxSlots)) return nullptr;
    return m->amax_dev + (size_t)it->second * kAmaxWays;
  };
  std::map<std::pair<const float*, int>, const void*> made;      // the RPN conv is shared by the five levels: one image per layout
  size_t need_partial = 0;
  for (size_t oi = 0; oi < m->ops.size(); ++oi) {
    const Op& op = m->ops[oi];
    const bool tail = m->op_tail > 0 && oi >= m->op_tail;
    if (op.kind == OP_PRE && pol.family == 2) {        // the preprocess kernel records the range of the padded frames
      ODT_CHECK(m->amax_used[0] < odt_model::kAmaxSlots, "too many conv outputs for the range slots");
      slot_of[m->image_pad.d] = m->amax_used[0];
      m->range_slot_name[m->amax_used[0]] = "preprocessed frames";
      m->pre_amax = m->amax_dev + (size_t)(m->amax_used[0]++) * kAmaxWays;
      continue;
    }
    if (op.kind == OP_ROI_HEAD && pol.family == 2 && m->roi_head.out_nhwc != nullptr && !m->knobs.off(K_ROI_AMAX)) {
      // the box head's RoI features: ROIAlign records their range, so that fc6 (K = 12544, a third of the box head's time on the
      // bf16x3 kernels) can take the fp16x2 kernels like every other layer (round 6; ODT_ROI_AMAX=0: A/B)
      const int g = tail ? 1 : 0;
      ODT_CHECK(m->amax_used[g] < odt_model::kAmaxSlots, "too many conv outputs for the range slots");
      const int slot = (tail ? odt_model::kAmaxSlots : 0) + m->amax_used[g]++;
      slot_of[m->roi_head.out_nhwc] = slot;
      m->roi_head.amax = m->amax_dev + (size_t)slot * kAmaxWays;
      m->range_slot_name[slot] = "roi_feat";
      continue;
    }
    if (op.kind == OP_RSE_APPLY) {
      // the SE block's output: the apply kernel records its range as a conv epilogue would, so that the next block's conv1 /
      // convshortcut (and the FPN lateral) keep the fp16x2 kernels
      slot_of.erase(op.rsa.out);
      if (pol.family != 2) continue;
      const int g = tail ? 1 : 0;
      ODT_CHECK(m->amax_used[g] < odt_model::kAmaxSlots, "too many conv outputs for the range slots");
      const int slot = (tail ? odt_model::kAmaxSlots : 0) + m->amax_used[g]++;
      slot_of[op.rsa.out] = slot;
      m->ops[oi].rsa.amax = m->amax_dev + (size_t)slot * kAmaxWays;
      for (const auto& kv : m->taps)
        if (kv.second.d == op.rsa.out) m->range_slot_name[slot] = kv.first + " (SE apply)";
      if (m->range_slot_name[slot].empty()) m->range_slot_name[slot] = "SE block output";
      continue;
    }
    if (op.kind == OP_GCONV) {
      // the grouped conv's output: the kernel records its range as a conv epilogue would, so that conv3 keeps the fp16x2 kernels
      slot_of.erase(op.gc.out);
      if (pol.family != 2) continue;
      const int g = tail ? 1 : 0;
      ODT_CHECK(m->amax_used[g] < odt_model::kAmaxSlots, "too many conv outputs for the range slots");
      const int slot = (tail ? odt_model::kAmaxSlots : 0) + m->amax_used[g]++;
      slot_of[op.gc.out] = slot;
      m->ops[oi].gc.out_amax = m->amax_dev + (size_t)slot * kAmaxWays;
      m->range_slot_name[slot] = "grouped conv2 output";
      continue;
    }
    if (op.kind == OP_DCONV) {
      // the deformable conv's output, likewise (the 18 offset channels feed that kernel alone: no slot)
      slot_of.erase(op.dc.out); slot_of.erase(op.dc.off);
      if (pol.family != 2) continue;
      const int g = tail ? 1 : 0;
      ODT_CHECK(m->amax_used[g] < odt_model::kAmaxSlots, "too many conv outputs for the range slots");
      const int slot = (tail ? odt_model::kAmaxSlots : 0) + m->amax_used[g]++;
      slot_of[op.dc.out] = slot;
      m->ops[oi].dc.out_amax = m->amax_dev + (size_t)slot * kAmaxWays;
      m->range_slot_name[slot] = "deformable conv2 output";
      continue;
    }
    if (op.kind == OP_GN) {
      // a GroupNorm layer's output -- the tensor the next convs read: the apply kernel records its range as a conv epilogue
      // would, so that they keep the fp16x2 kernels (the raw conv output in front has its own slot, which nothing reads)
      slot_of.erase(op.gn.out);
      if (pol.family != 2) continue;
      const int g = tail ? 1 : 0;
      ODT_CHECK(m->amax_used[g] < odt_model::kAmaxSlots, "too many conv outputs for the range slots");
      const int slot = (tail ? odt_model::kAmaxSlots : 0) + m->amax_used[g]++;
      slot_of[op.gn.out] = slot;
      m->ops[oi].gn.amax = m->amax_dev + (size_t)slot * kAmaxWays;
      for (const auto& kv : m->taps)
        if (kv.second.d == op.gn.out) m->range_slot_name[slot] = kv.first + " (GroupNorm)";
      if (m->range_slot_name[slot].empty()) m->range_slot_name[slot] = "GroupNorm output";
      continue;
    }
    if (op.kind == OP_GN_ROI) {
      // a ROI GroupNorm of the 4-conv box head, likewise: the next head conv and the fc read its output
      slot_of.erase(op.gnr.out);
      if (pol.family != 2) continue;
      const int g = tail ? 1 : 0;
      ODT_CHECK(m->amax_used[g] < odt_model::kAmaxSlots, "too many conv outputs for the range slots");
      const int slot = (tail ? odt_model::kAmaxSlots : 0) + m->amax_used[g]++;
      slot_of[op.gnr.out] = slot;
      m->ops[oi].gnr.amax = m->amax_dev + (size_t)slot * kAmaxWays;
      for (const auto& kv : m->taps)
        if (kv.second.d == op.gnr.out) m->range_slot_name[slot] = kv.first + " (ROI GroupNorm)";
      if (m->range_slot_name[slot].empty()) m->range_slot_name[slot] = "ROI GroupNorm output";
      continue;
    }
    if (op.kind == OP_RELATION_ATTN) {
      // a relation module's attention output, likewise: output_linear (K = 16 D) reads it
      slot_of.erase(op.ra.out);
      if (pol.family != 2) continue;
      const int g = tail ? 1 : 0;
      ODT_CHECK(m->amax_used[g] < odt_model::kAmaxSlots, "too many conv outputs for the range slots");
      const int slot = (tail ? odt_model::kAmaxSlots : 0) + m->amax_used[g]++;
      slot_of[op.ra.out] = slot;
      m->ops[oi].ra.amax = m->amax_dev + (size_t)slot * kAmaxWays;
      m->range_slot_name[slot] = op.rel == 0 ? "rm_r1_attn" : "rm_r2_attn";
      continue;
    }
    if (op.kind == OP_ATT_POOL || op.kind == OP_ATT_ADD) {
      // the attention branch of the box head, likewise: fastrcnn/att_trans reads the pooled RoI features, fastrcnn/outputs the sum
      const bool pool = op.kind == OP_ATT_POOL;
      const float* out = pool ? op.ap.out : op.aa.out;
      slot_of.erase(out);
      if (pol.family != 2) continue;
      const int g = tail ? 1 : 0;
      ODT_CHECK(m->amax_used[g] < odt_model::kAmaxSlots, "too many conv outputs for the range slots");
      const int slot = (tail ? odt_model::kAmaxSlots : 0) + m->amax_used[g]++;
      slot_of[out] = slot;
      (pool ? m->ops[oi].ap.amax : m->ops[oi].aa.amax) = m->amax_dev + (size_t)slot * kAmaxWays;
      m->range_slot_name[slot] = pool ? "att_pool" : "att_hidden";
      continue;
    }
    if (op.kind == OP_POOL || op.kind == OP_SUB2) {
      auto it = slot_of.find(op.in.d);
      if (it != slot_of.end()) slot_of[op.out.d] = it->second; else slot_of.erase(op.out.d);
      continue;
    }
    if (op.kind != OP_CONV) continue;
    ConvOp& c = m->convs[op.conv];
    c.p.in_amax = slot_ptr(c.p.in, tail);
    c.p.in2_amax = slot_ptr(c.p.in2, tail);
    const ConvChoice ch = conv_select(c.p, pol, m->knobs);
    const ConvKernelRow& row = conv_variant_row(ch.variant);
    if (row.family == CF_F32) { slot_of.erase(c.p.out); continue; }      // exact-f32 kernel (conv_finish picks its row): records no range
    conv_use_variant(c.p, ch.variant, ch.splitk, ch.reduce_blocks);
    const auto key = std::make_pair(c.p.wt, row.family * 1024 + row.bn);      // (the weight image's layout)
    auto it = made.find(key);
    if (it == made.end()) {
      float* img = m->alloc_f((conv_split_weight_bytes(c.p.Cout, conv_k(c.p)) + 3) / 4, false);
      ODT_CHECK(img != nullptr, "device allocation failed (split weights of " + c.name + ")");
      if (conv_make_split_weights(c.p, img, 0)) return 1;
      it = made.emplace(key, img).first;
    }
    conv_attach_weights(c.p, it->second);
    {
      // non-temporal hints on the loads of data that one workgroup reads once -- residual chunks (1), the activations of a 1x1
      // layer with a single n-tile (2) -- keep them from pushing the weights and the re-read tensors out of L2 / MALL: same-box
      // A/B at b=8 1080p 30.8 -> 29.8 ms of conv time, res4 conv1 275 -> 317 TF (profiles/r03_h2_nt_ab.txt; 4: large-output
      // stores, measured no gain).  ODT_CONV_NT overrides the mask (A/B).
      int nt = 3;
      nt = (int)m->knobs.get_long(K_CONV_NT, nt);
      c.p.debug |= (nt & 7) << 10;
    }
    {
      const bool per_wave = m->knobs.get(K_AMAX_PER_WAVE).c0 == '1';
      if (per_wave) c.p.debug |= 0x4000;      // A/B: range record per wave instead of per workgroup
    }
    if (row.family == CF_H2) {
      ++m->convs_h2;
      const bool norot = m->knobs.off(K_CONV_H2_ROT);
      if (norot) c.p.debug |= 0x100;          // A/B: every workgroup walks the K slices in the same order
    }
    need_partial = std::max(need_partial, conv_split_partial_bytes(c.p));
    // the output's slot (split-K layers: the combine pass records it, one atomic per block -- one per WAVE cost that short
    // memory-bound kernel 2x); only where the fp16x2 kernels may read it
    if (c.p.out != nullptr && pol.family == 2) {
      auto so = slot_of.find(c.p.out);
      int slot;
      if (so != slot_of.end() && (so->second >= odt_model::kAmaxSlots) == tail) slot = so->second;
      else {
        ODT_CHECK(m->amax_used[tail] < odt_model::kAmaxSlots, "too many conv outputs for the range slots");
        slot = (tail ? odt_model::kAmaxSlots : 0) + m->amax_used[tail]++;
        slot_of[c.p.out] = slot;
      }
      c.p.out_amax = m->amax_dev + (size_t)slot * kAmaxWays;
      if (m->range_slot_name[slot].empty()) m->range_slot_name[slot] = c.name;
    }
  }
  if (need_partial > 0) {
    // split-K scratch: the layers of one stream run one after another and share a buffer -- but the tail ops (box-head
    // FCs ...) of forward i run on the side stream UNDER the trunk of forward i+1 (tail overlap), so the two groups get
    // a buffer each
    std::vector<char> in_tail(m->convs.size(), 0);
    bool tail = false;
    for (const Op& op : m->ops) {
      if (op.kind == OP_PROPOSALS) tail = true;
      if (op.kind == OP_CONV && tail) in_tail[op.conv] = 1;
    }
    size_t need[2] = {0, 0};
    for (size_t i = 0; i < m->convs.size(); ++i)
      need[in_tail[i]] = std::max(need[in_tail[i]], conv_split_partial_bytes(m->convs[i].p));
    float* part[2] = {nullptr, nullptr};
    for (int g = 0; g < 2; ++g) {
      if (need[g] == 0) continue;
      part[g] = m->alloc_f((need[g] + 3) / 4, false);
      ODT_CHECK(part[g] != nullptr, "device allocation failed (split-K partial sums)");
    }
    for (size_t i = 0; i < m->convs.size(); ++i)
      if (conv_split_partial_bytes(m->convs[i].p) > 0) m->convs[i].p.partial = part[in_tail[i]];
  }
  ODT_HIP(hipDeviceSynchronize());
  return 0;
}


// ---- RPN head folded into the RPN conv's epilogue --------------------------------------------------------------------
// rpn/conv0@pL (3x3, 256 -> 256, ReLU) is followed by rpn/head@pL (1x1, 256 -> 3 logits || 12 deltas) and nothing else
// reads its output (models.py:979-1009).  Where the 3x3 conv runs on a conv_split3 kernel whose n-tile is the whole
// Cout (256) and has no split-K, the head is evaluated on the staged C tile in that kernel's epilogue (exact-f32 MFMA):
// the [M,256] tensor is neither written nor read back (2.1 GB at P2, b = 8) and the N = 15 launch disappears.
// ODT_FUSE_RPN_HEAD=0 keeps the two launches (A/B).  Called after attach_split_weights, before plan_arena.
int fuse_rpn_heads(odt_model* m) {
  m->conv_fused.assign(m->convs.size(), 0);
  if (m->knobs.off(K_FUSE_RPN_HEAD)) return 0;
  const HostTensor* W = find_w(m, "__rpnhead/W");
  const HostTensor* Bv = find_w(m, "__rpnhead/b");
  if (W == nullptr || Bv == nullptr) return 0;
  const float *hw = nullptr, *hb = nullptr;
  for (size_t oi = 0; oi + 1 < m->ops.size(); ++oi) {
    Op& oa = m->ops[oi]; Op& ob = m->ops[oi + 1];
    if (oa.kind != OP_CONV || ob.kind != OP_CONV) continue;
    ConvOp& a = m->convs[oa.conv]; ConvOp& b = m->convs[ob.conv];
    if (a.name.compare(0, 10, "rpn/conv0@") != 0 || b.name.compare(0, 9, "rpn/head@") != 0) continue;
    const ConvParams& bp = b.p;
    ConvParams& ap = a.p;
    const ConvKernelRow& ar = conv_variant_row(ap.variant);
    const bool ok = ap.wt_split != nullptr && (ar.family == CF_SPLIT3 || ar.family == CF_H2) && ar.bn == 256 && ap.Cout == 256 && ap.splitk <= 1 &&
                    ap.res_mode == 0 && ap.in2 == nullptr && ap.relu <= 1 && bp.in == ap.out && bp.kh == 1 && bp.kw == 1 &&
                    bp.Cin == 256 && bp.Cout == 15 && bp.out_ldc == 16 && bp.stride == 1 && bp.res_mode == 0 && bp.relu == 0 &&
                    bp.out_oy == 0 && bp.out_ox == 0 && bp.out_H == bp.Ho && bp.out_W == bp.Wo && bp.Ho == ap.Ho && bp.Wo == ap.Wo &&
                    ap.out_oy == 0 && ap.out_ox == 0 && ap.out_H == ap.Ho && ap.out_W == ap.Wo && (int)W->data.size() == 256 * 15;
    if (!ok) continue;
    if (hw == nullptr) {
      std::vector<float> v((size_t)256 * 16, 0.f), vb(16, 0.f);
      for (int c = 0; c < 256; ++c)
        for (int j = 0; j < 15; ++j) v[(size_t)c * 16 + j] = W->data[(size_t)c * 15 + j];
      for (int j = 0; j < 15; ++j) vb[j] = Bv->data[j];
      if (upload_raw(m, v, &hw) || upload_raw(m, vb, &hb)) return 1;
    }
    ap.head_wt = hw; ap.head_bias = hb; ap.head_out = bp.out; ap.head_ldc = bp.out_ldc;
    ap.out = nullptr;                      // nothing else reads the 256-channel tensor
    ap.out_amax = nullptr;
    ob.skip = true;
    m->conv_fused[ob.conv] = 1;
  }
  return 0;
}

// does anything but ops a and b -- another op, or (taps) a tap -- name tensor t?  What a fusion asks before it drops t.
static bool used_elsewhere(odt_model* m, const void* t, size_t a, size_t b, bool taps) {
  bool other = false;
  for (size_t k = 0; k < m->ops.size() && !other; ++k) {
    if (k == a || k == b) continue;
    visit_op_ptrs(m, k, [&](auto& ptr) { if ((const void*)ptr == t) other = true; });
  }
  if (taps) for (const auto& kv : m->taps) if (kv.second.d == t) other = true;
  return other;
}

// ---- bottleneck tail folded into the 3x3 conv's kernel ----------------------------------------------------------------
// block/conv2 (3x3, ch -> ch, BN, ReLU) is read by block/conv3 (1x1, ch -> 4 ch, BN, + shortcut, ReLU) and by nothing else
// (nn.py:503-521).  Where conv2 runs on conv_h2k_kernel with its whole Cout in one 256-wide n-tile (res4 at b >= 4 @1080p)
// and conv3 is a plain dense 1x1 (conv_h2f_fusable), conv3 is evaluated from conv2's accumulators inside that kernel
// (conv_h2k.hip: h2f_tail): conv2's [M,256] tensor is neither written nor read back, conv3's launch -- prologue, A stream,
// its own lock-step store phase behind an idle matrix pipe -- disappears, and conv3's operand gets its power of two per
// pixel row instead of per tensor.  ODT_FUSE_BOTTLENECK=0 keeps the two launches (A/B).  Called after
// attach_split_weights, before plan_arena.
int fuse_bottleneck_tails(odt_model* m) {
  if (m->conv_fused.size() < m->convs.size()) m->conv_fused.resize(m->convs.size(), 0);
  const char e0 = m->knobs.get(K_FUSE_BOTTLENECK).c0;      // A/B: 0 off | 1 only the 256-wide blocks (res4) | 2 + the 128-wide (res3) | otherwise every fusable block
  if (e0 == '0') return 0;
  const int min_cout = e0 == '1' ? 256 : (e0 == '2' ? 128 : 64);
  if (m->policy.arith == 0 || m->policy.family != 2) return 0;
  // SE blocks stay as they are: the fused tail never materialises conv2's output, which the gate pools, and its epilogue has no gate
  if (m->cfg.use_se) return 0;
  // basic and ResNeXt blocks have no dense 3x3 + 1x1 pair
  if (m->cfg.block_kind != 0) return 0;
  // GroupNorm stands between conv2 and conv3: conv2's whole output must exist before its statistics do
  if (m->cfg.use_gn) return 0;
  std::map<const float*, const void*> made;
  for (size_t oi = 0; oi + 1 < m->ops.size(); ++oi) {
    Op& oa = m->ops[oi]; Op& ob = m->ops[oi + 1];
    if (oa.kind != OP_CONV || ob.kind != OP_CONV || oa.skip || ob.skip) continue;
    ConvOp& a = m->convs[oa.conv]; ConvOp& b = m->convs[ob.conv];
    if (a.p.Cout < min_cout) continue;
    if (!conv_h2f_fusable(a.p, b.p)) continue;
    // nothing else may read conv2's output (taps: a keep_taps handle exposes no stage tensor under this name, see add_conv)
    if (used_elsewhere(m, a.p.out, oi, oi + 1, true)) continue;
    auto it = made.find(b.p.wt);
    if (it == made.end()) {
      float* img = m->alloc_f((conv_h2f_weight_bytes(b.p.Cout, b.p.Cin) + 3) / 4, false);
      ODT_CHECK(img != nullptr, "device allocation failed (fused 1x1 weights of " + b.name + ")");
      if (conv_make_h2f_weights(b.p.wt, b.p.Cout, b.p.Cin, img, 0)) return 1;
      it = made.emplace(b.p.wt, img).first;
    }
    conv_h2f_fuse(a.p, b.p, it->second);
    if (m->knobs.off(K_FUSE_ROT)) a.p.debug |= 0x100;     // A/B: 0 = every workgroup walks the output column chunks in the same order
    ob.skip = true;
    m->conv_fused[ob.conv] = 2;
    ++m->convs_h2f;
  }
  ODT_HIP(hipDeviceSynchronize());
  return 0;
}

// ---- res2 identity bottlenecks as one kernel per block ------------------------------------------------------------------
// block/conv1 (1x1, 256 -> 64, ReLU) -> block/conv2 (3x3, 64 -> 64, ReLU; already carrying the fused conv3 + shortcut + ReLU of
// fuse_bottleneck_tails) where the shortcut is conv1's input and nothing else reads conv1's output: conv_block_kernel
// (conv_block.hip) keeps conv1's output as an 18 x 18 pixel patch in LDS per 16 x 16 output pixels.  conv1's [M, 64] tensor is
// neither written nor read back, x is read from HBM once instead of twice, conv1's launch disappears, and conv2's operand
// gets its power of two per tile instead of per tensor.  conv2's record stays the launching record (its op becomes an
// OP_BLOCK) and keeps its row of the kernel table; conv1's and conv3's ops are skipped.  A record that upload_conv_records
// would cut into batch ranges (b = 24 @1080p) keeps the two launches.  A/B: profiles/block_fusion_res2_ab.txt.
// ODT_FUSE_BLOCK=0 keeps the two launches, 2 fuses without the kernel's first-round stagger (A/B).  Called after fuse_bottleneck_tails, before fuse_stem and plan_arena.
static int conv_batch_chunks(const ConvParams& p, double limit);
int fuse_bottleneck_blocks(odt_model* m) {
  if (m->knobs.off(K_FUSE_BLOCK)) return 0;
  if (m->policy.arith == 0 || m->policy.family != 2 || m->cfg.use_se || m->cfg.block_kind != 0) return 0;
  if (m->cfg.use_gn) return 0;      // (three normalisations inside the block)
  if (m->conv_fused.size() < m->convs.size()) m->conv_fused.resize(m->convs.size(), 0);
  double limit = 2147483648.0;
  if (m->knobs.get(K_CONV_CHUNK_BYTES).d > 0) limit = m->knobs.get(K_CONV_CHUNK_BYTES).d;
  std::map<const float*, const void*> made;
  for (size_t oi = 0; oi + 2 < m->ops.size(); ++oi) {
    Op& o1 = m->ops[oi]; Op& o2 = m->ops[oi + 1]; Op& o3 = m->ops[oi + 2];
    if (o1.kind != OP_CONV || o2.kind != OP_CONV || o3.kind != OP_CONV || o1.skip || o2.skip || !o3.skip) continue;
    if (m->conv_fused[o3.conv] != 2) continue;
    ConvOp& c1 = m->convs[o1.conv]; ConvOp& c2 = m->convs[o2.conv];
    if (c2.p.variant != CV_H2KF_256x64 || c2.p.f_out != m->convs[o3.conv].p.out || !conv_block_fits(c1.p, c2.p)) continue;
    // nothing else may read conv1's output
    if (used_elsewhere(m, c1.p.out, oi, oi + 1, true)) continue;
    ConvParams q = c2.p;
    q.in = c1.p.in; q.in_ldc = c1.p.in_ldc;
    if (conv_batch_chunks(q, limit) != 1 || conv_batch_chunks(c1.p, limit) != 1) continue;
    auto it = made.find(c2.p.wt);
    if (it == made.end()) {
      float* img = m->alloc_f((conv_split_weight_bytes(64, 9 * 64) + 3) / 4, false);
      ODT_CHECK(img != nullptr, "device allocation failed (block weights of " + c2.name + ")");
      if (conv_make_h2p_weights(c2.p, img, 0)) return 1;
      it = made.emplace(c2.p.wt, img).first;
    }
    conv_block_fuse(c2.p, c1.p, it->second);
    if (m->knobs.get(K_FUSE_BLOCK).c0 == '2') c2.p.debug |= 0x200;      // A/B: no first-round stagger
    o1.skip = true;
    m->conv_fused[o1.conv] = 3;
    o2.kind = OP_BLOCK;
    ++m->blocks_fused;
  }
  ODT_HIP(hipDeviceSynchronize());
  return 0;
}

// ---- conv0 + pool0 in one kernel ---------------------------------------------------------------------------------------
// pool0 reads conv0's map and nothing else does (nn.py:860-896): where conv0 runs on the fp16x2 family the pair becomes one
// launch of conv_stem_kernel (a 39 x 36 patch of the frame per 8 x 7 pooled pixels, split once into LDS; the [B,544,960,64] map
// -- 1.07 GB written and read back at b=8 -- never exists).  Bit-identical.  ODT_FUSE_STEM=0 keeps the two launches (A/B).
// Called after attach_split_weights, before plan_arena.
int fuse_stem(odt_model* m) {
  if (m->knobs.off(K_FUSE_STEM)) return 0;
  if (m->policy.arith == 0 || m->policy.family != 2) return 0;
  if (m->cfg.use_gn) return 0;      // (conv0's GroupNorm stands between conv0 and pool0)
  for (size_t oi = 0; oi + 1 < m->ops.size(); ++oi) {
    Op& oa = m->ops[oi]; Op& ob = m->ops[oi + 1];
    if (oa.kind != OP_CONV || ob.kind != OP_POOL || oa.skip || ob.skip) continue;
    ConvParams& ap = m->convs[oa.conv].p;
    if (ob.in.d != ap.out || ap.out == nullptr || !conv_stem_fits(ap) || ap.out_oy != 0 || ap.out_ox != 0 || ap.out_H != ap.Ho || ap.out_W != ap.Wo ||
        ob.in.h != ap.Ho || ob.in.w != ap.Wo || ob.in.C != 64 || ob.out.H != (ap.Ho + 1 - 3) / 2 + 1 || ob.out.W != (ap.Wo + 1 - 3) / 2 + 1 ||
        ob.out.C < 64 || (double)ap.B * ob.out.H * ob.out.W * ob.out.C * 4.0 >= 2147483648.0) continue;
    // nothing else may read the conv map (a keep_taps handle exposes it as "conv0"; arena handles keep no stage tensor: odt_tap
    // refuses the transient ones)
    if (used_elsewhere(m, ap.out, oi, oi + 1, !m->arena_on)) continue;
    // the conv map no longer exists: an arena handle must neither reserve memory for its stage name nor hand it out
    for (auto it = m->taps.begin(); it != m->taps.end();) { if (it->second.d == ap.out) it = m->taps.erase(it); else ++it; }
    conv_stem_fuse(ap, ob.out.d, ob.out.H, ob.out.W, ob.out.C);
    if (m->knobs.get(K_STEM_GRID).set) ap.debug |= ((int)m->knobs.get(K_STEM_GRID).i & 0x3ff) << 20;   // test knob: workgroups of the launch
    ob.skip = true;
    m->stem_fused = 1;
  }
  return 0;
}

// ---- GroupNorm scratch ------------------------------------------------------------------------------------------------
// The plan's GroupNorm layers run one after another on the compute stream, all of them in the trunk: they share one buffer of
// partial sums, one of per-channel factors and one of statistics, each sized for the largest layer.  A layer whose statistics
// are tapped keeps the buffers it already has.  Called once all ops exist, before plan_arena.
int attach_group_norm_scratch(odt_model* m) {
  size_t need_part = 0, need_ab = 0;
  for (const Op& op : m->ops) {
    if (op.kind != OP_GN) continue;
    const GroupNormParams& p = op.gn;
    need_part = std::max(need_part, (size_t)p.B * kGnGroups * group_norm_parts(p.h, p.w, p.C, p.chunks) * 2);
    need_ab = std::max(need_ab, (size_t)p.B * 2 * p.C);
  }
  if (need_part == 0) return 0;
  double* part = reinterpret_cast<double*>(m->alloc_f(need_part * 2, false));
  float* ab = m->alloc_f(need_ab, false);
  float* stats = m->alloc_f((size_t)m->cfg.batch * kGnGroups * 2, false);
  ODT_CHECK(part && ab && stats, "device allocation failed (GroupNorm scratch)");
  for (Op& op : m->ops) {
    if (op.kind != OP_GN) continue;
    op.gn.part = part; op.gn.ab = ab;
    if (op.gn.mean == nullptr) { op.gn.mean = stats; op.gn.var = stats + (size_t)m->cfg.batch * kGnGroups; }
  }
  return 0;
}

// ---- activation arena -----------------------------------------------------------------------------------------------
// ops [op_tail, end) of forward i (selection / ROIAlign / box head / NMS / features) may run on the side stream under ops
// [0, op_first_fpn) of forward i+1 (run_plan: tail overlap); 0 / 0 when the graph has no such split
void find_overlap_points(odt_model* m) {
  m->op_first_fpn = m->op_tail = 0;
  if (m->cfg.graph == ODT_GRAPH_EFFNET) return;
  for (size_t i = 0; i < m->ops.size(); ++i) {
    if (m->ops[i].kind == OP_PROPOSALS) { m->op_tail = i; break; }
    if (m->op_first_fpn == 0 && m->ops[i].kind == OP_CONV && m->convs[m->ops[i].conv].name.compare(0, 4, "fpn/") == 0)
      m->op_first_fpn = i;
  }
  if (m->op_tail == 0 || m->op_first_fpn == 0 || m->op_first_fpn >= m->op_tail) m->op_first_fpn = m->op_tail = 0;
}

// Lay the virtual stage tensors out in (at most) two arenas by live range and rewrite the plan's pointers.
// Region 1 holds what the tail ops touch (so that forward i's tail and forward i+1's early trunk never share memory);
// within a region a tensor takes the lowest offset not occupied by a tensor whose [first, last] range intersects its own
// (largest tensors first).  Called once, before the conv parameter records go to the device.
int plan_arena(odt_model* m) {
  if (!m->arena_on || m->vt.empty()) return 0;
  find_overlap_points(m);
  const int nops = (int)m->ops.size();
  for (int oi = 0; oi < nops; ++oi)
    visit_op_ptrs(m, (size_t)oi, [&](auto& p) {
      if (p == nullptr || !m->is_virtual((const void*)p)) return;
      odt_model::VTensor& v = m->vt[m->vt_index((const void*)p)];
      v.first = std::min(v.first, oi); v.last = std::max(v.last, oi);
    });
  const bool split = m->op_tail > 0;
  std::vector<char> tapped(m->vt.size(), 0);
  for (const auto& kv : m->taps)
    if (kv.second.d != nullptr && m->is_virtual(kv.second.d)) tapped[m->vt_index(kv.second.d)] = 1;
  for (size_t i = 0; i < m->vt.size(); ++i) {
    auto& v = m->vt[i];
    if (v.last < 0 && !tapped[i]) { v.bytes = 0; v.first = v.last = 0; }     // no op touches it (its producer was fused away)
    if (v.last < 0) { v.first = 0; v.last = nops - 1; }          // never referenced by an op (tap only): keep it apart
    v.region = split && v.last >= (int)m->op_tail ? 1 : 0;
    // forward i + 1 waits for forward i's tail only in front of op_first_fpn: what the tail reads must not be (re)written earlier
    ODT_CHECK(v.region == 0 || v.bytes == 0 || v.first >= (int)m->op_first_fpn || tapped[i],
              "activation arena: a tensor the tail ops read is produced before the FPN stage (tail overlap would race)");
    if (v.region == 1) v.last = nops - 1;                        // readable after the forward (appearance features / taps of the pyramid)
  }
  std::vector<int> order(m->vt.size());
  for (size_t i = 0; i < order.size(); ++i) order[i] = (int)i;
  std::sort(order.begin(), order.end(), [&](int a, int b) {
    return m->vt[a].bytes != m->vt[b].bytes ? m->vt[a].bytes > m->vt[b].bytes : a < b;
  });
  std::vector<int> placed;
  for (int id : order) {
    odt_model::VTensor& v = m->vt[id];
    // candidates: offset 0 and the end of every conflicting placed tensor; take the lowest that fits
    std::vector<std::pair<size_t, size_t>> busy;     // [begin, end) of placed tensors of this region alive at the same time
    for (int q : placed) {
      const odt_model::VTensor& u = m->vt[q];
      if (u.region == v.region && u.first <= v.last && v.first <= u.last) busy.emplace_back(u.off, u.off + u.bytes);
    }
    std::sort(busy.begin(), busy.end());
    size_t off = 0;
    for (const auto& b : busy) {
      if (off + v.bytes <= b.first) break;
      off = std::max(off, b.second);
    }
    v.off = off;
    m->arena_bytes[v.region] = std::max(m->arena_bytes[v.region], off + v.bytes);
    placed.push_back(id);
  }
  for (int r = 0; r < 2; ++r) {
    if (m->arena_bytes[r] == 0) continue;
    m->arena[r] = m->alloc_f(m->arena_bytes[r] / sizeof(float), false);
    ODT_CHECK(m->arena[r] != nullptr, "device allocation failed (activation arena): " + g_err);
  }
  auto fix = [&](auto& p) {
    if (p == nullptr || !m->is_virtual((const void*)p)) return;
    const odt_model::VTensor& v = m->vt[m->vt_index((const void*)p)];
    const size_t within = (size_t)((uintptr_t)p - odt_model::kVirtBase) - v.voff;
    p = reinterpret_cast<std::remove_reference_t<decltype(p)>>(reinterpret_cast<char*>(m->arena[v.region]) + v.off + within);
  };
  // taps first (they still hold virtual addresses: remember which of them do not outlive a forward)
  for (auto& kv : m->taps) {
    if (kv.second.d != nullptr && m->is_virtual(kv.second.d)) {
      const odt_model::VTensor& v = m->vt[m->vt_index(kv.second.d)];
      if (v.region == 0 && !(v.first == 0 && v.last == nops - 1)) m->transient_taps.insert(kv.first);
    }
    fix(kv.second.d);
  }
  for (size_t oi = 0; oi < m->ops.size(); ++oi) visit_op_ptrs(m, oi, fix);
  fix(m->image_pad.d);
  // every pointer a launched conv dereferences must be real memory by now (a field visit_op_ptrs does not enumerate would
  // still hold its virtual address)
  for (size_t oi = 0; oi < m->ops.size(); ++oi) {
    const Op& op = m->ops[oi];
    if ((op.kind != OP_CONV && op.kind != OP_BLOCK) || op.skip) continue;
    const ConvParams& c = m->convs[op.conv].p;
    for (const void* q : {(const void*)c.in, (const void*)c.res, (const void*)c.out, (const void*)c.in2, (const void*)c.head_out,
                          (const void*)c.f_res, (const void*)c.f_out, (const void*)c.b_in})
      ODT_CHECK(q == nullptr || !m->is_virtual(q), "activation arena: unmapped pointer left in " + m->convs[op.conv].name);
  }
  return 0;
}

// conv parameter records in device memory (the kernels read their ConvParams from there), finished and checked here: every
// launch choice is in the record, and the records do not change after this.  The conv kernels address
// their tensors through buffer descriptors with 32-bit offsets: a launch whose input / output / residual tensor would
// reach 2 GiB (b = 16 @1080p: conv0's output, the res2 tensors, P2) is cut into equal batch ranges, each with its own
// record whose pointers start at that range's first image -- every image's arithmetic is unchanged.
// (ODT_CONV_CHUNK_BYTES: test knob that lowers the limit so that small plans exercise the chunked path.)
static int conv_batch_chunks(const ConvParams& p, double limit) {
  auto fits = [&](int n) {
    const double b = (double)(p.B / n);
    return b * p.in_Ha * p.in_Wa * p.in_ldc * 4.0 < limit && b * p.out_H * p.out_W * p.out_ldc * 4.0 < limit &&
           (p.res_mode == 0 || b * p.res_H * p.res_W * p.res_ldc * 4.0 < limit) &&
           (p.in2 == nullptr || b * p.in2_Ha * p.in2_Wa * p.in2_ldc * 4.0 < limit) &&
           (p.f_wt == nullptr || (b * p.Ho * p.Wo * p.f_out_ldc * 4.0 < limit && (p.f_res == nullptr || b * p.Ho * p.Wo * p.f_res_ldc * 4.0 < limit)));
  };
  for (int n = 1; n <= p.B; ++n)
    if (p.B % n == 0 && fits(n)) return n;
  return p.B;           // (one image per launch; launch_conv reports it if even that is too large)
}

int upload_conv_records(odt_model* m) {
  double limit = 2147483648.0;
  if (m->knobs.get(K_CONV_CHUNK_BYTES).d > 0) limit = m->knobs.get(K_CONV_CHUNK_BYTES).d;
  m->conv_recs.clear(); m->conv_rec0.clear(); m->conv_nrec.clear();
  std::vector<char> launched(m->convs.size(), 0);
  for (const Op& op : m->ops)
    if ((op.kind == OP_CONV || op.kind == OP_BLOCK) && !op.skip) launched[op.conv] = 1;
  for (size_t ci = 0; ci < m->convs.size(); ++ci) {
    const ConvOp& c = m->convs[ci];
    const ConvParams& p = c.p;
    const int n = conv_batch_chunks(p, limit), bc = p.B / n;
    m->conv_rec0.push_back((int)m->conv_recs.size());
    m->conv_nrec.push_back(n);
    for (int k = 0; k < n; ++k) {
      ConvParams q = p;
      const size_t b0 = (size_t)k * bc;
      q.B = bc;
      q.in = p.in + b0 * p.in_Ha * p.in_Wa * p.in_ldc;
      if (p.out != nullptr) q.out = p.out + b0 * p.out_H * p.out_W * p.out_ldc;
      if (p.res != nullptr) q.res = p.res + b0 * p.res_H * p.res_W * p.res_ldc;
      if (p.in2 != nullptr) q.in2 = p.in2 + b0 * p.in2_Ha * p.in2_Wa * p.in2_ldc;
      if (p.head_out != nullptr) q.head_out = p.head_out + b0 * p.Ho * p.Wo * p.head_ldc;
      if (p.f_out != nullptr) q.f_out = p.f_out + b0 * p.Ho * p.Wo * p.f_out_ldc;
      if (p.f_res != nullptr) q.f_res = p.f_res + b0 * p.Ho * p.Wo * p.f_res_ldc;
      if (launched[ci] && conv_finish(q, m->knobs)) { g_err = c.name + ": " + g_err; return 1; }
      m->conv_recs.push_back(q);
    }
    if (n > 1) ++m->chunked_convs;
  }
  m->bufs.emplace_back(new DevBuf());
  if (m->bufs.back()->alloc(m->conv_recs.size() * sizeof(ConvParams))) return 1;
  m->convs_dev = (ConvParams*)m->bufs.back()->p;
  ODT_HIP(hipMemcpy(m->convs_dev, m->conv_recs.data(), m->conv_recs.size() * sizeof(ConvParams), hipMemcpyHostToDevice));
  return 0;
}

}  // namespace odt
