// Static plan of the reference's Mask_RCNN_FPN / Mask_RCNN_FPN_multi inference graphs:
// preprocess -> ResNet-101-dilated + FPN -> RPN -> proposals -> ROIAlign -> box head -> detections -> appearance features
// (+ mask head).  reference nn.py:843-1014, models.py:979-1108, :2058-2408.  build_plan (at the end) lists the stages; each
// stage function takes the tensors it consumes and returns those it produces.
#include "odt_model.hpp"

#define g_err (::odt::last_error())

namespace odt {
namespace {

constexpr int kFpnStrides[5] = {4, 8, 16, 32, 64};

// ---- GroupNorm (--use_gn; nn.py:81-108).  The scope of the gamma / beta that follow conv `name` under odt_config.use_gn: X/gn
// where the BN graph has X/bn (the backbone), fpn/gn_cN and fpn/gn_pN behind the FPN convs (nn.py:987-1009); "" for every other
// layer (RPN, heads) and without the flag
std::string gn_scope(const odt_model* m, const std::string& name, bool has_bn) {
  if (!m->cfg.use_gn) return "";
  if (has_bn) return name + "/gn";
  for (const char* pre : {"fpn/lateral_1x1_", "fpn/posthoc_3x3_"})
    if (name.compare(0, 16, pre) == 0) return "fpn/gn_" + name.substr(16);
  return "";
}

// Append GroupNorm of y over scope/{gamma,beta} with what a conv epilogue would carry: the residual (as ConvParams::res_mode),
// the ReLU, the output's offset (oy, ox) inside a zero-bordered tensor and its stage name.  Out of place: the normalised
// tensor is the one the next convs read and gets a range slot of its own (attach_split_weights).  keep_taps handles expose
// the statistics of conv0's and fpn/gn_p2's layer as "conv0/gn_mean", "conv0/gn_var", "fpn/gn_p2/gn_mean", "fpn/gn_p2/gn_var"
int add_group_norm(odt_model* m, const std::string& scope, const Tensor& y, int relu, const Tensor* res, int res_mode, int oy, int ox,
                   const std::string& tap, Tensor* out) {
  const int C = y.c;
  ODT_CHECK(relu == 0 || relu == 1, "GroupNorm: " + scope + " is followed by an activation other than ReLU");
  ODT_CHECK(C % kGnGroups == 0, "GroupNorm: " + scope + " has " + std::to_string(C) + " channels, not a multiple of 32");
  const HostTensor* g = find_w(m, scope + "/gamma");
  const HostTensor* b = find_w(m, scope + "/beta");
  ODT_CHECK(g && b, "missing GroupNorm variables " + scope + "/{gamma,beta} (odt_config.use_gn)");
  ODT_CHECK(g->data.size() == (size_t)C && b->data.size() == (size_t)C, "bad GroupNorm shapes for " + scope);
  if (make_tensor(m, tap, y.B, y.h + oy, y.w + ox, C, out, oy != 0 || ox != 0)) return 1;
  Op op; op.kind = OP_GN; op.out = *out;
  GroupNormParams& p = op.gn;
  std::memset(&p, 0, sizeof(p));
  if (upload_raw(m, g->data, &p.gamma) || upload_raw(m, b->data, &p.beta)) return 1;
  p.x = y.d; p.out = out->d;
  p.B = y.B; p.h = y.h; p.w = y.w; p.C = C; p.Ha = y.H; p.Wa = y.W; p.ldc = y.C;
  p.oH = out->H; p.oW = out->W; p.out_ldc = out->C; p.oy = oy; p.ox = ox;
  if (res != nullptr && res_mode != 0) { p.res = res->d; p.res_mode = res_mode; p.res_H = res->H; p.res_W = res->W; p.res_ldc = res->C; }
  p.relu = relu; p.eps = 1e-5f;
  for (const char* s : {"conv0/gn", "fpn/gn_p2"}) {
    if (!m->cfg.keep_taps || scope != s) continue;
    p.mean = m->alloc_f((size_t)y.B * kGnGroups, true); p.var = m->alloc_f((size_t)y.B * kGnGroups, true);
    ODT_CHECK(p.mean && p.var, "device allocation failed (GroupNorm statistics of " + scope + ")");
    const std::string name = scope == "conv0/gn" ? "conv0" : scope;
    Tensor t{}; t.B = 1; t.H = t.h = 1; t.W = t.w = y.B; t.C = t.c = kGnGroups;
    t.d = p.mean; m->taps[name + "/gn_mean"] = t;
    t.d = p.var; m->taps[name + "/gn_var"] = t;
  }
  op.gnorm = m->gn_ops++;
  m->ops.push_back(op);
  return 0;
}

// Append GroupNorm per ROI of y [R,7,7,C] over scope/{gamma,beta} (the 4-conv box head under use_gn: behind the conv's ReLU,
// nothing behind it): one launch of group_norm_roi.hip, out of place like add_group_norm.  Not counted among the frame-level
// layers (gn_ops).  keep_taps handles expose the statistics of fastrcnn/gn0 as "head_conv0/gn_mean" / "head_conv0/gn_var" [R,32]
int add_group_norm_roi(odt_model* m, const std::string& scope, const Tensor& y, const std::string& tap, Tensor* out) {
  const int C = y.c;
  ODT_CHECK(C % kGnGroups == 0, "GroupNorm: " + scope + " has " + std::to_string(C) + " channels, not a multiple of 32");
  ODT_CHECK(y.H == y.h && y.W == y.w, "GroupNorm: the ROI tensor in front of " + scope + " is not dense");
  const HostTensor* g = find_w(m, scope + "/gamma");
  const HostTensor* b = find_w(m, scope + "/beta");
  ODT_CHECK(g && b, "missing GroupNorm variables " + scope + "/{gamma,beta} (odt_config.use_gn with use_conv_frcnn_head)");
  ODT_CHECK(g->data.size() == (size_t)C && b->data.size() == (size_t)C, "bad GroupNorm shapes for " + scope);
  if (make_tensor(m, tap, y.B, y.H, y.W, C, out)) return 1;
  Op op; op.kind = OP_GN_ROI; op.out = *out;
  RoiGroupNormParams& p = op.gnr;
  std::memset(&p, 0, sizeof(p));
  if (upload_raw(m, g->data, &p.gamma) || upload_raw(m, b->data, &p.beta)) return 1;
  p.x = y.d; p.out = out->d;
  p.R = y.B; p.hw = y.h * y.w; p.C = C; p.ldc = y.C; p.out_ldc = out->C; p.eps = 1e-5f;
  if (m->cfg.keep_taps && scope == "fastrcnn/gn0") {
    p.mean = m->alloc_f((size_t)y.B * kGnGroups, true); p.var = m->alloc_f((size_t)y.B * kGnGroups, true);
    ODT_CHECK(p.mean && p.var, "device allocation failed (GroupNorm statistics of " + scope + ")");
    Tensor t{}; t.B = 1; t.H = t.h = 1; t.W = t.w = y.B; t.C = t.c = kGnGroups;
    t.d = p.mean; m->taps[tap + "/gn_mean"] = t;
    t.d = p.var; m->taps[tap + "/gn_var"] = t;
  }
  op.gnroi = m->gn_roi_ops++;
  m->ops.push_back(op);
  return 0;
}

// upload the weights of the scope `c` is named after (W + folded BN where has_bn, W + b otherwise) and append the conv.  Under
// odt_config.use_gn a normalised layer is the conv as it is -- nothing folded, no activation, residual or offset -- followed by
// its GroupNorm, which carries them
int conv_layer(odt_model* m, ConvSpec c, bool has_bn, Tensor* out) {
  const std::string gn = gn_scope(m, c.name, has_bn);
  if (gn.empty()) {
    if (upload_conv(m, c.name, c.kh, c.kw, c.cin, c.cout, has_bn, &c.wt, &c.bias)) return 1;
    return add_conv(m, c, out);
  }
  ConvSpec raw = c;
  raw.relu = 0; raw.res = nullptr; raw.res_mode = 0; raw.oy = raw.ox = 0; raw.tap = "";
  if (upload_conv_plain(m, c.name, c.kh, c.kw, c.cin, c.cout, !has_bn, &raw.wt, &raw.bias)) return 1;
  Tensor y{};
  if (add_conv(m, raw, &y)) return 1;
  return add_group_norm(m, gn, y, c.relu, c.res, c.res_mode, c.oy, c.ox, c.tap, out);
}

// Two 1x1 layers over one input as one: the [cin, na] weights of scope `a` and the [cin, nb] weights of scope `b` side by side
// along Cout, their biases likewise, as the variables name/W and name/b
int concat_cout(odt_model* m, const std::string& a, int na, const std::string& b, int nb, int cin, const std::string& name) {
  const HostTensor* wa = find_w(m, a + "/W"); const HostTensor* ba = find_w(m, a + "/b");
  const HostTensor* wb = find_w(m, b + "/W"); const HostTensor* bb = find_w(m, b + "/b");
  ODT_CHECK(wa && ba && wb && bb, "missing " + a + " or " + b + " variables");
  ODT_CHECK(wa->data.size() == (size_t)cin * na && wb->data.size() == (size_t)cin * nb, "bad " + a + " / " + b + " shapes");
  const int n = na + nb;
  HostTensor v, vb;
  v.data.resize((size_t)cin * n); vb.data.resize(n);
  for (int i = 0; i < cin; ++i) {
    for (int j = 0; j < na; ++j) v.data[(size_t)i * n + j] = wa->data[(size_t)i * na + j];
    for (int j = 0; j < nb; ++j) v.data[(size_t)i * n + na + j] = wb->data[(size_t)i * nb + j];
  }
  for (int j = 0; j < na; ++j) vb.data[j] = ba->data[j];
  for (int j = 0; j < nb; ++j) vb.data[na + j] = bb->data[j];
  m->host_w[name + "/W"] = v; m->host_w[name + "/b"] = vb;
  return 0;
}

// One relation module of the box head (--add_relation_nn; relation_network nn.py:115-190 from models.py:1044-1054): out = f +
// RM(f, boxes) over the proposals of each image, f [1,1,B K,D].  Four launches: Q | K = f [query_linear/W | key_linear/W] as ONE
// 1x1 conv (no bias), the geometric bias and the attention (relation.hip), and output_linear over the [B K, 16 D] attention output
// as a 1x1 conv whose epilogue adds f -- a residual with no activation behind it, as the FPN's top-down sum has.  `geo` is the
// [B,16,K,Kp] bias buffer, shared by the two modules.  Stage names: `tap` (the sum) and `tap`_attn (the attention output)
int relation_module(odt_model* m, int index, const std::string& scope, const Tensor& f, const Tensor& props, const Tensor& geo,
                    const std::string& tap, Tensor* out) {
  const odt_config& cfg = m->cfg;
  const int B = cfg.batch, K = cfg.rpn_topk, D = cfg.head_dim, R = B * K;
  struct Var { const char* name; size_t elems; const char* shape; };
  const Var vars[7] = {{"geo_emb/W", (size_t)4 * kRelGeoDim, "[4,64]"}, {"geo_emb/b", (size_t)kRelGeoDim, "[64]"},
                       {"geo_conv/W", (size_t)kRelGeoDim * kRelHeads, "[1,1,64,16]"}, {"geo_conv/b", (size_t)kRelHeads, "[16]"},
                       {"query_linear/W", (size_t)D * D, "[D,D]"}, {"key_linear/W", (size_t)D * D, "[D,D]"},
                       {"output_linear/W", (size_t)kRelHeads * D * D, "[16 D,D]"}};
  const HostTensor* w[7];
  for (int i = 0; i < 7; ++i) {
    w[i] = find_w(m, scope + "/" + vars[i].name);
    ODT_CHECK(w[i] != nullptr, "missing relation variable " + scope + "/" + vars[i].name + " (odt_config.add_relation_nn)");
    ODT_CHECK(w[i]->data.size() == vars[i].elems, "bad shape for " + scope + "/" + vars[i].name + " (" + vars[i].shape + " with D = " +
                                                      std::to_string(D) + ")");
  }
  {   // [query_linear/W | key_linear/W] side by side along Cout
    HostTensor v; v.data.resize((size_t)D * 2 * D);
    for (int i = 0; i < D; ++i) {
      std::memcpy(&v.data[(size_t)i * 2 * D], &w[4]->data[(size_t)i * D], sizeof(float) * D);
      std::memcpy(&v.data[(size_t)i * 2 * D + D], &w[5]->data[(size_t)i * D], sizeof(float) * D);
    }
    m->host_w["__" + tap + "qk/W"] = v;
  }
  Tensor qk{};
  ConvSpec cq(scope + "/query_key_linear", f, D, 2 * D);
  if (upload_conv_plain(m, "__" + tap + "qk", 1, 1, D, 2 * D, false, &cq.wt, &cq.bias) || add_conv(m, cq, &qk)) return 1;
  m->host_w.erase("__" + tap + "qk/W");
  Op og; og.kind = OP_RELATION_GEO; og.rel = index;
  {
    std::vector<float> gw;
    for (int i = 0; i < 4; ++i) gw.insert(gw.end(), w[i]->data.begin(), w[i]->data.end());
    RelationGeoParams& g = og.rg;
    std::memset(&g, 0, sizeof(g));
    if (upload_raw(m, gw, &g.wts)) return 1;
    g.boxes = props.d; g.count = m->prop.nprops; g.bias = geo.d; g.B = B; g.K = K; g.Kp = geo.C;
  }
  m->ops.push_back(og);
  Tensor att{};
  if (make_tensor(m, tap + "_attn", 1, 1, R, kRelHeads * D, &att)) return 1;
  Op oa; oa.kind = OP_RELATION_ATTN; oa.rel = index; oa.out = att;
  {
    RelationAttnParams& a = oa.ra;
    std::memset(&a, 0, sizeof(a));
    a.q = qk.d; a.k = qk.d + D; a.qk_ldc = qk.C; a.v = f.d; a.v_ldc = f.C; a.bias = geo.d; a.count = m->prop.nprops; a.out = att.d;
    a.B = B; a.K = K; a.Kp = geo.C; a.D = D;
  }
  m->ops.push_back(oa);
  ++m->rel_modules;
  ConvSpec co(scope + "/output_linear", att, kRelHeads * D, D);
  co.res = &f; co.res_mode = 1; co.tap = tap;
  return upload_conv_plain(m, scope + "/output_linear", 1, 1, kRelHeads * D, D, false, &co.wt, &co.bias) || add_conv(m, co, out);
}

// The attention branch of the box head (--use_att_frcnn_head; fastrcnn_2fc_head, models.py:1064-1089 and :2682-2707), behind
// whichever `hidden` [1,1,B K,D] the configured head produced: out = hidden + relu(attended fastrcnn/att_trans/W + b), attended =
// sum over the 49 positions of feature * attention.  The attention map is conv2d(..., activation = softmax) over ONE channel: 1.0f
// for every finite logit, so the device sums the RoI features and does not evaluate that conv; fastrcnn/attention/{W,b} must be
// there, of the graph's shapes and finite (a non-finite one gives NaN rows in the reference).  Three launches: OP_ATT_POOL over
// `roi` (the [1,1,B K,49 FC] RoI features the head already read), att_trans as a 1x1 conv with bias and ReLU on the conv kernels,
// OP_ATT_ADD -- the add sits behind the ReLU, so it is not a conv residual.  Stage names: att_pool, att_trans, att_hidden
int attention_branch(odt_model* m, const Tensor& roi, const Tensor& hidden, Tensor* out) {
  const odt_config& cfg = m->cfg;
  const int FC = cfg.fpn_channels, D = cfg.head_dim, R = cfg.batch * cfg.rpn_topk;
  ODT_CHECK(FC % 4 == 0 && D % 4 == 0, "use_att_frcnn_head: fpn_channels and head_dim must be multiples of 4");
  ODT_CHECK(roi.W == R && roi.C == kRoiOut * kRoiOut * FC && hidden.W == R && hidden.c == D,
            "use_att_frcnn_head: the RoI features or the head's hidden vector are not [B K, ...] rows");
  struct Var { const char* name; size_t elems; std::string shape; };
  const Var vars[4] = {{"attention/W", (size_t)9 * FC, "[3,3," + std::to_string(FC) + ",1]"}, {"attention/b", 1, "[1]"},
                       {"att_trans/W", (size_t)FC * D, "[" + std::to_string(FC) + "," + std::to_string(D) + "]"},
                       {"att_trans/b", (size_t)D, "[" + std::to_string(D) + "]"}};
  for (const Var& v : vars) {
    const std::string name = std::string("fastrcnn/") + v.name;
    const HostTensor* w = find_w(m, name);
    ODT_CHECK(w != nullptr, "missing attention box head variable " + name + " (odt_config.use_att_frcnn_head)");
    ODT_CHECK(w->data.size() == v.elems, "bad shape for " + name + " (" + v.shape + ")");
    if (name.compare(0, 19, "fastrcnn/attention/") != 0) continue;
    for (float x : w->data)
      ODT_CHECK(std::isfinite(x), name + " holds a non-finite value: the reference's softmax over the map's one channel returns NaN "
                                         "there, not the 1.0 this path rests on (odt_config.use_att_frcnn_head)");
  }
  Tensor pooled{}, att{};
  if (make_tensor(m, "att_pool", 1, 1, R, FC, &pooled)) return 1;
  {
    Op op; op.kind = OP_ATT_POOL; op.out = pooled;
    std::memset(&op.ap, 0, sizeof(op.ap));
    op.ap.x = roi.d; op.ap.out = pooled.d; op.ap.R = R; op.ap.C = FC;
    m->ops.push_back(op);
  }
  ConvSpec ct("fastrcnn/att_trans", pooled, FC, D);
  ct.relu = 1; ct.tap = "att_trans";
  if (conv_layer(m, ct, false, &att)) return 1;
  m->att_conv = (int)m->convs.size() - 1;
  ODT_CHECK(att.C == D, "use_att_frcnn_head: the output of fastrcnn/att_trans is not dense");
  if (make_tensor(m, "att_hidden", 1, 1, R, D, out)) return 1;
  {
    Op op; op.kind = OP_ATT_ADD; op.out = *out;
    std::memset(&op.aa, 0, sizeof(op.aa));
    op.aa.h = hidden.d; op.aa.a = att.d; op.aa.out = out->d; op.aa.R = R; op.aa.D = D; op.aa.ldh = hidden.C;
    m->ops.push_back(op);
  }
  m->att_head = 1;
  return 0;
}

// ---- front end (nn.py:860-896; tf_pad_reverse => pad [3, 2 + pad_to_32]): image pad, conv0, pool0 -> the pooled map
int front_end(odt_model* m, Tensor* pool) {
  const int B = m->cfg.batch, H = m->cfg.height, W = m->cfg.width;
  const int ph = ceil_div(H, 32) * 32 - H, pw = ceil_div(W, 32) * 32 - W;
  const int Hp = 3 + H + 2 + ph, Wpl = 3 + W + 2 + pw;
  const int Ho0 = (Hp - 7) / 2 + 1, Wo0 = (Wpl - 7) / 2 + 1;
  const int Wp = 2 * Wo0 + 8;          // room for the 8th (zero-weight) tap of the last window
  m->Hp = Hp; m->Wp = Wp;
  if (make_tensor(m, "image_pad", B, Hp, Wp, 4, &m->image_pad)) return 1;
  m->frames_bytes = (size_t)B * H * W * 3 * sizeof(float);
  m->src_h = H; m->src_w = W;
  { m->bufs.emplace_back(new DevBuf()); if (m->bufs.back()->alloc(m->frames_bytes)) return 1;
    m->frames_dev.d = (float*)m->bufs.back()->p; }
  { Op op; op.kind = OP_PRE; m->ops.push_back(op); }

  // ---- conv0: 7x7 s2 VALID as a 7x1 conv over 8-tap x 4-channel rows (K = 7*32)
  ConvSpec c0("conv0", m->image_pad, 32, 64);
  c0.kh = 7; c0.stride = 2; c0.Ho = Ho0; c0.Wo = Wo0; c0.relu = 1; c0.tap = "conv0";
  {
    const HostTensor* W0 = find_w(m, "conv0/W");
    ODT_CHECK(W0 && W0->data.size() == (size_t)7 * 7 * 3 * 64, "missing/bad conv0/W");
    HostTensor v;   // virtual HWIO [7,1,32,64]
    v.data.assign((size_t)7 * 32 * 64, 0.f);
    for (int y = 0; y < 7; ++y)
      for (int x = 0; x < 7; ++x)
        for (int c = 0; c < 3; ++c)
          for (int o = 0; o < 64; ++o)
            v.data[((size_t)y * 32 + x * 4 + c) * 64 + o] = W0->data[(((size_t)y * 7 + x) * 3 + c) * 64 + o];
    m->host_w["__conv0v/W"] = v;
    if (m->cfg.use_gn) {      // conv0 -> GN -> ReLU (nn.py:859-862): the conv alone, conv0/gn behind it
      if (upload_conv_plain(m, "__conv0v", 7, 1, 32, 64, false, &c0.wt, &c0.bias)) return 1;
    } else {
      for (const char* s : {"gamma", "beta", "mean/EMA", "variance/EMA"}) {
        const HostTensor* t = find_w(m, std::string("conv0/bn/") + s);
        ODT_CHECK(t != nullptr, std::string("missing conv0/bn/") + s);
        m->host_w[std::string("__conv0v/bn/") + s] = *t;
      }
      if (upload_conv(m, "__conv0v", 7, 1, 32, 64, true, &c0.wt, &c0.bias)) return 1;
    }
  }
  Tensor x{};
  if (m->cfg.use_gn) {
    Tensor y{};
    c0.relu = 0; c0.tap = "";
    if (add_conv(m, c0, &y) || add_group_norm(m, "conv0/gn", y, 1, nullptr, 0, 0, 0, "conv0", &x)) return 1;
  } else if (add_conv(m, c0, &x)) return 1;
  // ---- pool0: pad top/left 1, 3x3 s2 VALID max
  const int Hq = (Ho0 + 1 - 3) / 2 + 1, Wq = (Wo0 + 1 - 3) / 2 + 1;
  if (make_tensor(m, "pool0", B, Hq, Wq, 64, pool)) return 1;
  { Op op; op.kind = OP_POOL; op.in = x; op.out = *pool; m->ops.push_back(op); }
  return 0;
}

// ---- ResNet groups (nn.py:459-588, 898-936).  A block function reads x (x.c channels) and returns the block's output
struct Block {
  std::string pre, tap;      // variable scope; stage name of the output ("": none)
  int ch, stride, dil;       // the group's width, the block's stride and dilation
  bool deform;               // --use_deformable puts a deformable conv2 here
};

// resnet_shortcut (nn.py:551-566) as a conv of its own: 1x1, stride 2 VALID on x[:, :, :-1, :-1] (nn.py:555-556), BN, no ReLU
int shortcut_conv(odt_model* m, const std::string& pre, const Tensor& x, int cout, int stride, int Ho, int Wo, Tensor* s) {
  Tensor xc = x;
  if (stride == 2) { xc.h = x.h - 1; xc.w = x.w - 1; }
  ODT_CHECK((xc.h - 1) / stride + 1 == Ho && (xc.w - 1) / stride + 1 == Wo, "shortcut / block geometry mismatch in " + pre);
  ConvSpec c(pre + "/convshortcut", xc, x.c, cout);
  c.stride = stride; c.Ho = Ho; c.Wo = Wo;
  return conv_layer(m, c, true, s);
}

// The tail of a bottleneck or ResNeXt block (nn.py:503-521): conv3 (1x1 on t2, to cout channels, BN) + shortcut(x), ReLU
int conv3_tail(odt_model* m, const Block& b, const Tensor& x, const Tensor& t2, int cout, Tensor* y) {
  const int cin = x.c, Ho = t2.h, Wo = t2.w;
  // (under GroupNorm conv3 and the shortcut conv are normalised apart, each with its own statistics: two convs, the
  // normalised shortcut added as conv3's plain residual)
  if (cin != cout && !m->knobs.off(K_FUSE_SHORTCUT) && !m->cfg.use_gn) {
    // stage entry: conv3(t2) + convshortcut(x[::stride]) as one K-concatenated GEMM -- saves the
    // shortcut tensor's write + read and one launch (shortcut[:, :, :-1, :-1] of nn.py:555-556
    // never matters: the stride-2 samples stop at 2 * (Ho - 1) <= h - 2)
    ODT_CHECK((x.h - b.stride) / b.stride + 1 == Ho && (x.w - b.stride) / b.stride + 1 == Wo, "shortcut / conv2 geometry mismatch in " + b.pre);
    ConvSpec c(b.pre + "/conv3+shortcut", t2, t2.c, cout);
    if (upload_conv_cat(m, b.pre + "/conv3", t2.c, b.pre + "/convshortcut", cin, cout, &c.wt, &c.bias)) return 1;
    c.relu = 1; c.in2 = &x; c.cin2 = cin; c.in2_stride = b.stride; c.tap = b.tap;
    return add_conv(m, c, y);
  }
  Tensor sc = x;
  if (cin != cout) {
    sc = Tensor{};
    if (shortcut_conv(m, b.pre, x, cout, b.stride, Ho, Wo, &sc)) return 1;
  }
  ConvSpec c(b.pre + "/conv3", t2, t2.c, cout);
  c.res = &sc; c.res_mode = 1; c.relu = 1; c.tap = b.tap;
  return conv_layer(m, c, true, y);
}

// resnet_basicblock (nn.py:439-456; --resnet18 / --resnet34): conv1 3x3 stride s 'SAME' + BN + ReLU, conv2 3x3 + BN,
// + shortcut (the input itself where cin == ch, which includes group0/block0), ReLU.  `dilations` is ignored there
int basic_block(odt_model* m, const Block& b, const Tensor& x, Tensor* y) {
  const int ch = b.ch;
  int Ho, Wo, pt, pl;
  same_pad(x.h, 3, b.stride, &Ho, &pt); same_pad(x.w, 3, b.stride, &Wo, &pl);
  Tensor t1{}, sc = x;
  ConvSpec c1(b.pre + "/conv1", x, x.c, ch);
  c1.kh = c1.kw = 3; c1.stride = b.stride; c1.pad_t = pt; c1.pad_l = pl; c1.Ho = Ho; c1.Wo = Wo; c1.relu = 1;
  if (conv_layer(m, c1, true, &t1)) return 1;
  if (x.c != ch) {
    sc = Tensor{};
    if (shortcut_conv(m, b.pre, x, ch, b.stride, Ho, Wo, &sc)) return 1;
  }
  ODT_CHECK(sc.H == Ho && sc.W == Wo && sc.h == Ho && sc.w == Wo, "basic block: shortcut / conv2 geometry mismatch in " + b.pre);
  ConvSpec c2(b.pre + "/conv2", t1, ch, ch);
  c2.kh = c2.kw = 3; c2.pad_t = c2.pad_l = 1; c2.res = &sc; c2.res_mode = 1; c2.relu = 1; c2.tap = b.tap;
  return conv_layer(m, c2, true, y);
}

// resnext_32x4d_bottleneck (nn.py:524-549; --use_resnext): conv1 1x1 to 2 ch, conv2 3x3 in 32 groups with the block's
// stride AND dilation under 'SAME' (conv_group.hip), conv3 1x1 to 4 ch + the bottleneck's shortcut, ReLU
int resnext_block(odt_model* m, const Block& b, const Tensor& x, Tensor* y) {
  const int C2 = b.ch * 2;
  int Ho, Wo, pt, pl;
  same_pad(x.h, 2 * b.dil + 1, b.stride, &Ho, &pt); same_pad(x.w, 2 * b.dil + 1, b.stride, &Wo, &pl);
  Tensor t1{}, t2{};
  ConvSpec c1(b.pre + "/conv1", x, x.c, C2);
  c1.relu = 1;
  if (conv_layer(m, c1, true, &t1)) return 1;
  ODT_CHECK(t1.C == C2 && t1.H == t1.h && t1.W == t1.w, "ResNeXt block: conv1's output is not dense in " + b.pre);
  if (make_tensor(m, "", x.B, Ho, Wo, C2, &t2)) return 1;
  Op og; og.kind = OP_GCONV;
  GroupConvParams& gp = og.gc;
  if (upload_group_conv(m, b.pre + "/conv2", C2, &gp.wt, &gp.bias)) return 1;
  gp.in = t1.d; gp.out = t2.d; gp.out_amax = nullptr;
  gp.B = x.B; gp.H = t1.h; gp.W = t1.w; gp.C = C2; gp.Ho = Ho; gp.Wo = Wo;
  gp.stride = b.stride; gp.dil = b.dil; gp.pad_t = pt; gp.pad_l = pl; gp.relu = 1;
  og.gconv = m->gconv_ops++;
  m->ops.push_back(og);
  return conv3_tail(m, b, x, t2, b.ch * 4, y);
}

// resnet_bottleneck (nn.py:487-521): conv1 1x1 to ch, conv2 3x3 with the block's stride and dilation (deformable where the
// reference has it), conv3 1x1 to 4 ch (gated in an SE block) + shortcut, ReLU
int bottleneck_block(odt_model* m, const Block& b, const Tensor& x, Tensor* y) {
  const int B = x.B, ch = b.ch, dil = b.dil;
  const std::string& pre = b.pre;
  Tensor t1{}, t2{};
  ConvSpec c1(pre + "/conv1", x, x.c, ch);
  c1.relu = 1;
  if (conv_layer(m, c1, true, &t1)) return 1;
  if (b.deform) {
    // conv2_offset (3x3, C -> 18, bias) + the deformable conv2 (no bias, BN or ReLU): conv_deform.hip.  With dilation 2 the
    // reference pads this block's conv2 output once more (nn.py:493-497), ceil(h / 2) + 1 against the shortcut's h / 2: its
    // graph does not build
    ODT_CHECK(dil == 1, "use_deformable with use_dilations: the reference graph does not build (" + pre +
              " would be deformable and dilated); set use_dilations = 0");
    ODT_CHECK(ch == 128 || ch == 256 || ch == 512, "deformable conv: C must be 128, 256 or 512 (" + pre + ")");
    const int Ho = (x.h + 1) / 2, Wo = (x.w + 1) / 2;
    Tensor toff{};
    if (make_tensor(m, pre + "/conv2_offset", B, Ho, Wo, 18, &toff)) return 1;
    if (make_tensor(m, pre + "/conv2", B, Ho, Wo, ch, &t2)) return 1;
    Op od; od.kind = OP_DCONV;
    DeformConvParams& dp = od.dc;
    if (upload_deform_conv(m, pre, ch, &dp.wt_off, &dp.b_off, &dp.wt)) return 1;
    dp.in = t1.d; dp.off = toff.d; dp.out = t2.d; dp.out_amax = nullptr;
    dp.B = B; dp.H = t1.h; dp.W = t1.w; dp.Ha = t1.H; dp.Wa = t1.W; dp.ldc = t1.C; dp.C = ch; dp.Ho = Ho; dp.Wo = Wo;
    od.dconv = m->dconv_ops++;
    m->ops.push_back(od);
  } else {
    ConvSpec c2(pre + "/conv2", t1, ch, ch);
    c2.kh = c2.kw = 3; c2.dil = dil; c2.relu = 1;
    if (b.stride == 2) {
      const int keff = 2 * dil + 1;
      c2.stride = 2; c2.pad_t = c2.pad_l = 1;
      c2.Ho = (x.h + 1 - keff) / 2 + 1; c2.Wo = (x.w + 1 - keff) / 2 + 1;
      c2.oy = c2.ox = dil != 1 ? 1 : 0;       // nn.py:493-497 second pad, after BN+ReLU
    } else {
      c2.pad_t = c2.pad_l = dil;
    }
    if (conv_layer(m, c2, true, &t2)) return 1;
  }
  // (SE blocks gate conv3's output but not the shortcut: the two cannot share one GEMM)
  if (!m->cfg.use_se) return conv3_tail(m, b, x, t2, ch * 4, y);
  // squeeze-excitation (nn.py:506-517): the gate from the pooled t2 (conv3 + BN folded into fc1: upload_se_gate), conv3
  // without residual / ReLU, then out = max(y * gate + shortcut, 0) in one pass (resnet_se.hip)
  const int Ho = t2.h, Wo = t2.w;
  Tensor sc = x, y3{};
  if (x.c != ch * 4) {
    sc = Tensor{};
    if (shortcut_conv(m, pre, x, ch * 4, b.stride, Ho, Wo, &sc)) return 1;
  }
  ODT_CHECK(t2.C == ch && t2.H == Ho && t2.W == Wo, "SE block: conv2's output is not dense in " + pre);
  ODT_CHECK(sc.C == ch * 4 && sc.H == Ho && sc.W == Wo && sc.h == Ho && sc.w == Wo,
            "SE block: shortcut / conv3 geometry mismatch in " + pre);
  Op og; og.kind = OP_RSE_GATE;
  ResSeParams& gp = og.rse;
  gp.t2 = t2.d; gp.B = B; gp.HW = Ho * Wo; gp.ch = ch; gp.r = ch / 4; gp.cout = ch * 4; gp.gate_ld = ch * 4;
  if (upload_se_gate(m, pre, ch, &gp.w1, &gp.b1, &gp.w2t, &gp.b2)) return 1;
  gp.part = m->alloc_f((size_t)B * channel_mean_splits(gp.HW, ch, B) * ch, false);
  gp.mean = m->alloc_f((size_t)B * ch, false);
  gp.rvec = m->alloc_f((size_t)B * gp.r, false);
  gp.gate = m->alloc_f((size_t)B * gp.gate_ld, true);
  ODT_CHECK(gp.part && gp.mean && gp.rvec && gp.gate, "device allocation failed (SE gate of " + pre + ")");
  m->ops.push_back(og);
  { Tensor gt{}; gt.d = gp.gate; gt.B = 1; gt.H = gt.h = 1; gt.W = gt.w = B; gt.C = gt.c = gp.gate_ld; m->taps[pre + "/se_gate"] = gt; }
  if (conv_layer(m, ConvSpec(pre + "/conv3", t2, ch, ch * 4), true, &y3)) return 1;
  if (make_tensor(m, b.tap, B, Ho, Wo, ch * 4, y)) return 1;
  Op oa; oa.kind = OP_RSE_APPLY; oa.out = *y;
  ResSeApplyParams& ap = oa.rsa;
  ap.y = y3.d; ap.sc = sc.d; ap.gate = gp.gate; ap.out = y->d; ap.amax = nullptr;
  ap.B = B; ap.HW = Ho * Wo; ap.C = ch * 4; ap.ldc = ch * 4; ap.gate_ld = gp.gate_ld;
  m->ops.push_back(oa);
  ++m->se_blocks;
  return 0;
}

int backbone(odt_model* m, Tensor x, Tensor cfeat[4]) {
  const odt_config& cfg = m->cfg;
  const int feats[4] = {64, 128, 256, 512};
  ODT_CHECK(cfg.block_kind >= 0 && cfg.block_kind <= 2, "odt_config.block_kind must be 0 (bottleneck), 1 (basic) or 2 (ResNeXt-32x4d)");
  ODT_CHECK(cfg.block_kind == 0 || !cfg.use_se, "squeeze-excitation is built for the plain bottleneck only (block_kind 0)");
  ODT_CHECK(!cfg.use_deformable || (cfg.block_kind == 0 && !cfg.use_se),
            "use_deformable is built for the plain bottleneck only (block_kind 0, no squeeze-excitation)");
  ODT_CHECK(!cfg.use_gn || (cfg.block_kind == 0 && !cfg.use_se && !cfg.use_deformable),
            "use_gn is built for the plain bottleneck only (block_kind 0, no squeeze-excitation, no deformable conv)");
  for (int g = 0; g < 4; ++g) {
    const int cnt = cfg.num_blocks[g];
    for (int i = 0; i < cnt; ++i) {
      Block b;
      b.pre = "group" + std::to_string(g) + "/block" + std::to_string(i);
      b.tap = (i == cnt - 1) ? "c" + std::to_string(g + 2) : (i == 0 ? b.pre : "");
      b.ch = feats[g];
      b.stride = (i == 0 && g > 0) ? 2 : 1;
      b.dil = (g == 3 && cfg.use_dilations && i >= cnt - 3) ? 2 : 1;
      // --use_deformable (nn.py:469-485, 574-585): the stride-2 bottleneck that opens a stage, where block 0 is among the
      // group's last three blocks
      b.deform = cfg.use_deformable != 0 && b.stride == 2 && cnt <= 3;
      Tensor y{};
      if (cfg.block_kind == 1 ? basic_block(m, b, x, &y) : cfg.block_kind == 2 ? resnext_block(m, b, x, &y) : bottleneck_block(m, b, x, &y))
        return 1;
      x = y;
    }
    cfeat[g] = x;
  }
  return 0;
}

// ---- FPN (nn.py:947-1014): lateral 1x1 (+ nearest-2x top-down add), posthoc 3x3, P6 -> P2..P6
int fpn(odt_model* m, const Tensor cfeat[4], Tensor P[5]) {
  const int FC = m->cfg.fpn_channels;
  Tensor lat[4];
  for (int l = 3; l >= 0; --l) {
    const Tensor* res = l < 3 ? &lat[l + 1] : nullptr;
    if (res) ODT_CHECK(res->H * 2 == cfeat[l].h && res->W * 2 == cfeat[l].w, "FPN levels are not exact 2x");
    ConvSpec c("fpn/lateral_1x1_c" + std::to_string(l + 2), cfeat[l], cfeat[l].c, FC);
    c.res = res; c.res_mode = 2;
    if (conv_layer(m, c, false, &lat[l])) return 1;
  }
  for (int l = 0; l < 4; ++l) {
    ConvSpec c("fpn/posthoc_3x3_p" + std::to_string(l + 2), lat[l], FC, FC);
    c.kh = c.kw = 3; c.pad_t = c.pad_l = 1;
    if (conv_layer(m, c, false, &P[l])) return 1;
  }
  {
    const int h6 = (P[3].h - 1) / 2 + 1, w6 = (P[3].w - 1) / 2 + 1;
    if (make_tensor(m, "p6", m->cfg.batch, h6, w6, FC, &P[4])) return 1;
    Op op; op.kind = OP_SUB2; op.in = P[3]; op.out = P[4]; m->ops.push_back(op);
  }
  // slice_feature_and_anchors (models.py:372-400): P2..P4 cropped to ceil(H / stride)
  for (int l = 0; l < 3; ++l) {
    const int th = (int)std::ceil((float)m->cfg.height * (float)(1.0 / kFpnStrides[l]));
    const int tw = (int)std::ceil((float)m->cfg.width * (float)(1.0 / kFpnStrides[l]));
    ODT_CHECK(th <= P[l].H && tw <= P[l].W, "sliced feature larger than the feature map");
    P[l].h = th; P[l].w = tw;
  }
  for (int l = 0; l < 5; ++l) m->taps["p" + std::to_string(l + 2)] = P[l];
  return 0;
}

// ---- RPN head (models.py:979-1009), class(3) + box(12) merged into one 15-channel 1x1
int rpn_head(odt_model* m, const Tensor P[5], Tensor rpn_out[5]) {
  const int FC = m->cfg.fpn_channels;
  const float *w_r0, *b_r0, *w_r1, *b_r1;
  if (upload_conv(m, "rpn/conv0", 3, 3, FC, FC, false, &w_r0, &b_r0)) return 1;
  if (concat_cout(m, "rpn/class", 3, "rpn/box", 12, FC, "__rpnhead")) return 1;
  if (upload_conv(m, "__rpnhead", 1, 1, FC, 15, false, &w_r1, &b_r1)) return 1;
  for (int l = 0; l < 5; ++l) {
    Tensor t{};
    ConvSpec c0("rpn/conv0@p" + std::to_string(l + 2), P[l], FC, FC);
    c0.wt = w_r0; c0.bias = b_r0; c0.kh = c0.kw = 3; c0.pad_t = c0.pad_l = 1; c0.relu = 1;
    if (add_conv(m, c0, &t)) return 1;
    ConvSpec c1("rpn/head@p" + std::to_string(l + 2), t, FC, 15);
    c1.wt = w_r1; c1.bias = b_r1; c1.out_ldc = kRpnCh; c1.tap = "rpn" + std::to_string(l + 2);
    if (add_conv(m, c1, &rpn_out[l])) return 1;
  }
  return 0;
}

// ---- proposals: m->prop, the [B, K, 4] boxes in `props` and their counts in m->prop.nprops
int proposals(odt_model* m, const Tensor rpn_out[5], Tensor* props) {
  const odt_config& cfg = m->cfg;
  const int B = cfg.batch, K = cfg.rpn_topk, L = 5;
  ProposalParams& pp = m->prop;
  pp.nlevels = L; pp.graph = cfg.graph; pp.B = B; pp.K = K; pp.img_h = cfg.height; pp.img_w = cfg.width;
  pp.nms_thresh = cfg.rpn_nms_thresh; pp.decode_clip = cfg.rpn_decode_clip;
  for (int l = 0; l < L; ++l) {
    const HostTensor* a = find_w(m, "anchors/lvl" + std::to_string(l));
    ODT_CHECK(a != nullptr && a->shape.size() == 4 && a->shape[2] == 3 && a->shape[3] == 4 &&
              a->shape[0] == a->shape[1], "missing/bad anchors/lvl" + std::to_string(l));
    ODT_CHECK(a->shape[0] >= rpn_out[l].h && a->shape[0] >= rpn_out[l].w, "anchor field smaller than feature map");
    const float* d;
    if (upload_raw(m, a->data, &d)) return 1;
    pp.lvl[l].rpn = rpn_out[l].d; pp.lvl[l].anchors = d; pp.lvl[l].h = rpn_out[l].h; pp.lvl[l].w = rpn_out[l].w;
    pp.lvl[l].field = (int)a->shape[0];
    ODT_CHECK(rpn_out[l].H == rpn_out[l].h && rpn_out[l].W == rpn_out[l].w, "rpn output must be dense");
  }
  const size_t per = (size_t)B * L * K;
  pp.cand_boxes = m->alloc_f(per * 4, true); pp.cand_scores = m->alloc_f(per, true);
  pp.lvl_boxes = m->alloc_f(per * 4, true); pp.lvl_scores = m->alloc_f(per, true);
  pp.cand_count = (int*)m->alloc_f((size_t)B * L, true); pp.lvl_count = (int*)m->alloc_f((size_t)B * L, true);
  if (make_tensor(m, "proposals", 1, B, K, 4, props, true)) return 1;
  pp.props = props->d;
  pp.nprops = (int*)m->alloc_f(B, true);
  pp.chunk_keys = (unsigned long long*)m->alloc_f((size_t)B * proposal_total_chunks(pp) * K * 2, true);
  ODT_CHECK(pp.cand_boxes && pp.cand_scores && pp.lvl_boxes && pp.lvl_scores && pp.cand_count &&
            pp.lvl_count && pp.nprops && pp.chunk_keys, "device allocation failed (proposals)");
  { Op op; op.kind = OP_PROPOSALS; m->ops.push_back(op); }
  return 0;
}

// ---- ROIAlign over P2..P5 -> box head (models.py:465-485, 1030-1108) -> the [B K, C || 4 C] class logits and box deltas
int box_head(odt_model* m, const Tensor P[5], const Tensor& props, Tensor* hout) {
  const odt_config& cfg = m->cfg;
  const int B = cfg.batch, K = cfg.rpn_topk, FC = cfg.fpn_channels, D = cfg.head_dim, C = cfg.num_class;
  Tensor roi{}; if (make_tensor(m, "roi_feat", 1, 1, B * K, 49 * FC, &roi, true)) return 1;
  RoiAlignParams& rh = m->roi_head;
  std::memset(&rh, 0, sizeof(rh));
  for (int l = 0; l < 4; ++l) {
    rh.feat[l] = P[l].d; rh.h[l] = P[l].h; rh.w[l] = P[l].w; rh.ldc[l] = P[l].C;
    rh.alloc_h[l] = P[l].H; rh.alloc_w[l] = P[l].W; rh.inv_stride[l] = (float)(1.0 / kFpnStrides[l]);
  }
  rh.C = FC; rh.boxes = props.d; rh.box_ind = nullptr; rh.per_image = K; rh.count = m->prop.nprops;
  rh.R_cap = B * K; rh.out_nhwc = roi.d;
  m->roi_final = rh;
  { Op op; op.kind = OP_ROI_HEAD; m->ops.push_back(op); }

  // the dense layer behind the RoI tensor of `cin` channels: rows of W are flattened NCHW (c*49 + h*7 + w, nn.py:736-738); our
  // RoI rows are (h,w,c).  scope/{W,b} -> the variables `as`/{W,b}
  auto flat_dense = [&](const std::string& scope, int cin, const std::string& as) -> int {
    const HostTensor* w6 = find_w(m, scope + "/W");
    ODT_CHECK(w6 && w6->data.size() == (size_t)cin * 49 * D, "missing/bad " + scope + "/W");
    HostTensor v; v.data.resize(w6->data.size());
    for (int c = 0; c < cin; ++c)
      for (int s = 0; s < 49; ++s)
        std::memcpy(&v.data[((size_t)s * cin + c) * D], &w6->data[((size_t)c * 49 + s) * D], sizeof(float) * D);
    m->host_w[as + "/W"] = v;
    const HostTensor* b6 = find_w(m, scope + "/b"); ODT_CHECK(b6 != nullptr && b6->data.size() == (size_t)D, "missing/bad " + scope + "/b");
    m->host_w[as + "/b"] = *b6;
    return 0;
  };
  Tensor h6{}, h7{};
  // compacted rows: only the first nprops[b] rows of each image are meaningful
  if (cfg.use_conv_frcnn_head) {
    // --use_conv_frcnn_head (fastrcnn 4conv1fc: conv_frcnn_head, models.py:1110-1124, from :1038-1041 / :1133-1136 /
    // :2656-2659): four 3x3 'SAME' convs with ReLU over the [R,7,7,FC] RoI images -- under use_gn each followed by GroupNorm,
    // BEHIND the ReLU and with no activation of its own -- then ONE dense layer fastrcnn/fc + ReLU; no fc6 / fc7.  Rows past
    // nprops[b] are zero RoIs: finite through every layer, normalised like any other row
    const int DC = cfg.conv_head_dim, R = B * K;
    ODT_CHECK(cfg.add_relation_nn == 0, "add_relation_nn: not built with use_conv_frcnn_head (the reference ignores the flag there)");
    ODT_CHECK(DC >= 32 && DC <= 512 && DC % 32 == 0, "use_conv_frcnn_head: odt_config.conv_head_dim must be a multiple of 32 in [32, 512]");
    Tensor cur = roi;
    cur.B = R; cur.H = cur.h = kRoiOut; cur.W = cur.w = kRoiOut; cur.C = cur.c = FC;
    for (int k = 0; k < 4; ++k) {
      const std::string ks = std::to_string(k), scope = "fastrcnn/conv" + ks;
      const int cin = k == 0 ? FC : DC;
      const HostTensor* w = find_w(m, scope + "/W"); const HostTensor* b = find_w(m, scope + "/b");
      ODT_CHECK(w && b, "missing 4-conv box head variables " + scope + "/{W,b} (odt_config.use_conv_frcnn_head)");
      ODT_CHECK(w->data.size() == (size_t)9 * cin * DC && b->data.size() == (size_t)DC,
                "bad shapes for " + scope + " (W [3,3," + std::to_string(cin) + "," + std::to_string(DC) + "], b [" + std::to_string(DC) + "])");
      ConvSpec c(scope, cur, cin, DC);
      c.kh = c.kw = 3; c.pad_t = c.pad_l = 1; c.relu = 1;
      c.tap = cfg.use_gn ? "" : "head_conv" + ks;
      Tensor y{}, nx{};
      if (conv_layer(m, c, false, &y)) return 1;
      if (!cfg.use_gn) nx = y;
      else if (add_group_norm_roi(m, "fastrcnn/gn" + ks, y, "head_conv" + ks, &nx)) return 1;
      cur = nx;
    }
    ODT_CHECK(cur.C == DC && cur.H == kRoiOut && cur.W == kRoiOut, "4-conv box head: the last conv's output is not dense");
    Tensor flat = cur;                    // [R,7,7,DC] viewed as [1,1,R,49*DC]
    flat.B = 1; flat.H = flat.h = 1; flat.W = flat.w = R; flat.C = flat.c = 49 * DC;
    if (flat_dense("fastrcnn/fc", DC, "__headfc")) return 1;
    ConvSpec cf("fastrcnn/fc", flat, 49 * DC, D);
    cf.relu = 1; cf.tap = "head_fc";
    if (upload_conv(m, "__headfc", 1, 1, 49 * DC, D, false, &cf.wt, &cf.bias) || add_conv(m, cf, &h7)) return 1;
  } else {
    // --add_relation_nn (models.py:1044-1054): h6' = h6 + RM_r1(h6, boxes) feeds fc7, h7' = h7 + RM_r2(h7, boxes) the output layers
    const bool rel = cfg.add_relation_nn != 0;
    Tensor geo{};
    if (rel) {
      ODT_CHECK(cfg.graph == ODT_GRAPH_SINGLE, "add_relation_nn: built for the single-image graph only (the batched graph of the reference "
                                               "calls the head without boxes)");
      ODT_CHECK(K <= kRelMaxK, "add_relation_nn: rpn_topk = " + std::to_string(K) + " proposals per image, at most " + std::to_string(kRelMaxK));
      ODT_CHECK(D % 64 == 0 && D <= kRelMaxD, "add_relation_nn: head_dim = " + std::to_string(D) + ", not a multiple of 64 up to " +
                                                  std::to_string(kRelMaxD));
      if (make_tensor(m, "", B, kRelHeads, K, relation_kp(K), &geo)) return 1;
    }
    if (flat_dense("fastrcnn/fc6", FC, "__fc6")) return 1;
    ConvSpec c6("fastrcnn/fc6", roi, 49 * FC, D);
    c6.relu = 1; c6.tap = "fc6";
    if (upload_conv(m, "__fc6", 1, 1, 49 * FC, D, false, &c6.wt, &c6.bias) || add_conv(m, c6, &h6)) return 1;
    Tensor h6r{}, h7r{};
    if (rel) { if (relation_module(m, 0, "fastrcnn/RM_r1", h6, props, geo, "rm_r1", &h6r)) return 1; h6 = h6r; }
    ConvSpec c7("fastrcnn/fc7", h6, D, D);
    c7.relu = 1; c7.tap = "fc7";
    if (conv_layer(m, c7, false, &h7)) return 1;
    if (rel) { if (relation_module(m, 1, "fastrcnn/RM_r2", h7, props, geo, "rm_r2", &h7r)) return 1; h7 = h7r; }
  }
  if (cfg.use_att_frcnn_head) { Tensor ha{}; if (attention_branch(m, roi, h7, &ha)) return 1; h7 = ha; }
  if (concat_cout(m, "fastrcnn/outputs/class", C, "fastrcnn/outputs/box", 4 * C, D, "__headout")) return 1;
  ConvSpec co("fastrcnn/outputs", h7, D, C * 5);
  co.out_ldc = (C * 5 + 3) / 4 * 4; co.tap = "head_out";
  return upload_conv(m, "__headout", 1, 1, D, C * 5, false, &co.wt, &co.bias) || add_conv(m, co, hout);
}

// ---- detection tail: m->det
int detection_tail(odt_model* m, const Tensor& props, const Tensor& hout) {
  const odt_config& cfg = m->cfg;
  const int B = cfg.batch, K = cfg.rpn_topk, C = cfg.num_class, per_im = cfg.result_per_im;
  DetectParams& dp = m->det;
  std::memset(&dp, 0, sizeof(dp));
  dp.graph = cfg.graph; dp.B = B; dp.K = K; dp.C = C; dp.head_out = hout.d; dp.ld = hout.C;
  dp.props = props.d; dp.nprops = m->prop.nprops; dp.img_h = cfg.height; dp.img_w = cfg.width;
  for (int i = 0; i < 4; ++i) dp.reg_w[i] = cfg.bbox_reg_weights[i];
  dp.decode_clip = cfg.head_decode_clip; dp.score_thresh = cfg.result_score_thresh;
  dp.nms_thresh = cfg.head_nms_thresh; dp.per_im = per_im;
  Tensor dec{}, prb{};
  if (make_tensor(m, "decoded_boxes", 1, B * K, C - 1, 4, &dec, true)) return 1;
  if (make_tensor(m, "label_probs", 1, 1, B * K, C, &prb, true)) return 1;
  dp.dec_boxes = dec.d; dp.probs = prb.d;
  dp.cls_keep = (int*)m->alloc_f((size_t)B * (C - 1) * per_im, true);
  dp.cls_count = (int*)m->alloc_f((size_t)B * (C - 1), true);
  dp.out_boxes = m->alloc_f((size_t)B * per_im * 4, true);
  dp.out_probs = m->alloc_f((size_t)B * per_im, true);
  dp.out_labels = (int*)m->alloc_f((size_t)B * per_im, true);
  dp.out_valid = (int*)m->alloc_f(B, true);
  ODT_CHECK(dp.cls_keep && dp.cls_count && dp.out_boxes && dp.out_probs && dp.out_labels && dp.out_valid,
            "device allocation failed (detections)");
  { Op op; op.kind = OP_DETECT; m->ops.push_back(op); }
  return 0;
}

// ---- appearance features: ROIAlign of the final boxes (models.py:971-973) + 7x7 mean
int appearance_features(odt_model* m) {
  const int B = m->cfg.batch, FC = m->cfg.fpn_channels, per_im = m->cfg.result_per_im;
  m->final_feat = m->alloc_f((size_t)B * per_im * FC * 49, true);
  m->final_pooled = m->alloc_f((size_t)B * per_im * FC, true);
  ODT_CHECK(m->final_feat && m->final_pooled, "device allocation failed (features)");
  RoiAlignParams& rf = m->roi_final;
  rf.boxes = m->det.out_boxes; rf.per_image = per_im; rf.count = m->det.out_valid; rf.R_cap = B * per_im;
  rf.out_nhwc = nullptr; rf.out_nchw = m->final_feat; rf.pooled = m->final_pooled;
  rf.pack_rows = 1;                      // fpn_box_feat is [M,...] over the valid detections of all images
  { Op op; op.kind = OP_ROI_FINAL; m->ops.push_back(op); }
  return 0;
}

// ---- Mask R-CNN head on the final boxes (--add_mask; models.py:932-962, 1173-1199): 14x14
// ROIAlign, 4 x (3x3 conv + ReLU), 2x2 stride-2 transposed conv + ReLU, 1x1 conv to the
// foreground classes, sigmoid of each detection's own class.  The transposed conv has no
// overlap (kernel == stride), so it runs as ONE 1x1 conv to 4 * dim sub-pixel channels
// (dy, dx, co); the following 1x1 conv treats [R,14,14,4*dim] as [R,14,56,dim] pixels and the
// pixel shuffle to 28x28 happens in mask_select_kernel.
int mask_head(odt_model* m) {
  const odt_config& cfg = m->cfg;
  const int B = cfg.batch, FC = cfg.fpn_channels, C = cfg.num_class, per_im = cfg.result_per_im;
  ODT_CHECK(cfg.graph == ODT_GRAPH_SINGLE, "add_mask: built for the single-image graph only");
  const int MD = cfg.mask_dim > 0 ? cfg.mask_dim : 256;
  ODT_CHECK(MD % 32 == 0, "add_mask: mrcnn_head_dim must be a multiple of 32");
  const int R = B * per_im;
  Tensor mroi{};
  if (make_tensor(m, "mask_roi", R, 14, 14, FC, &mroi, true)) return 1;
  m->roi_mask = m->roi_final;
  m->roi_mask.out_nhwc = mroi.d; m->roi_mask.out_nchw = nullptr; m->roi_mask.pooled = nullptr;
  m->roi_mask.out_size = 14;
  { Op op; op.kind = OP_ROI_MASK; m->ops.push_back(op); }
  Tensor cur = mroi;
  for (int k = 0; k < 4; ++k) {
    ConvSpec c("maskrcnn/fcn" + std::to_string(k), cur, k == 0 ? FC : MD, MD);
    c.kh = c.kw = 3; c.pad_t = c.pad_l = 1; c.relu = 1; c.tap = "mask_fcn" + std::to_string(k);
    Tensor nx{};
    if (conv_layer(m, c, false, &nx)) return 1;
    cur = nx;
  }
  {   // Conv2DTranspose kernel [2,2,out,in] (nn.py:383-413) -> 1x1 conv [in][(dy,dx,out)]
    const HostTensor* wd = find_w(m, "maskrcnn/deconv/W"); const HostTensor* bd = find_w(m, "maskrcnn/deconv/b");
    ODT_CHECK(wd && bd, "missing maskrcnn/deconv variables");
    ODT_CHECK(wd->data.size() == (size_t)4 * MD * MD && bd->data.size() == (size_t)MD, "bad maskrcnn/deconv shapes");
    HostTensor v, vb; v.data.resize((size_t)MD * 4 * MD); vb.data.resize((size_t)4 * MD);
    for (int q = 0; q < 4; ++q)
      for (int co = 0; co < MD; ++co) {
        vb.data[(size_t)q * MD + co] = bd->data[co];
        for (int ci = 0; ci < MD; ++ci)
          v.data[(size_t)ci * 4 * MD + (size_t)q * MD + co] = wd->data[((size_t)q * MD + co) * MD + ci];
      }
    m->host_w["__maskdeconv/W"] = v; m->host_w["__maskdeconv/b"] = vb;
  }
  Tensor dc{};
  ConvSpec cd("maskrcnn/deconv", cur, MD, 4 * MD);
  cd.relu = 1; cd.tap = "mask_deconv";
  if (upload_conv(m, "__maskdeconv", 1, 1, MD, 4 * MD, false, &cd.wt, &cd.bias) || add_conv(m, cd, &dc)) return 1;
  Tensor dv = dc;                       // [R,14,14,4*MD] viewed as [R,14,56,MD]
  dv.W = dv.w = 56; dv.C = MD; dv.c = MD;
  Tensor ml{};
  ConvSpec cl("maskrcnn/conv", dv, MD, C - 1);
  cl.out_ldc = (C - 1 + 3) / 4 * 4; cl.tap = "mask_logits";
  if (conv_layer(m, cl, false, &ml)) return 1;
  m->final_masks = m->alloc_f((size_t)R * 784, true);
  ODT_CHECK(m->final_masks != nullptr, "device allocation failed (masks)");
  MaskSelectParams& ms = m->mask_sel;
  ms.logits = ml.d; ms.ld = ml.C; ms.labels = m->det.out_labels; ms.valid = m->det.out_valid; ms.B = B;
  ms.per_image = per_im; ms.masks = m->final_masks;
  { Op op; op.kind = OP_MASK_SELECT; m->ops.push_back(op); }
  return 0;
}

}  // namespace

// Build the whole static plan (called from odt_finalize_weights).
int build_plan(odt_model* m) {
  m->arena_on = m->cfg.keep_taps == 0;
  if (m->cfg.graph == ODT_GRAPH_EFFNET) return build_plan_effnet(m);
  Tensor pool{}, cfeat[4], P[5], rpn_out[5], props{}, hout{};
  if (front_end(m, &pool)) return 1;
  if (backbone(m, pool, cfeat)) return 1;
  if (fpn(m, cfeat, P)) return 1;
  if (rpn_head(m, P, rpn_out)) return 1;
  if (proposals(m, rpn_out, &props)) return 1;
  if (box_head(m, P, props, &hout)) return 1;
  if (detection_tail(m, props, hout)) return 1;
  if (appearance_features(m)) return 1;
  if (m->cfg.add_mask && mask_head(m)) return 1;
  if (attach_split_weights(m)) return 1;
  if (fuse_rpn_heads(m)) return 1;
  if (fuse_bottleneck_tails(m)) return 1;
  if (fuse_bottleneck_blocks(m)) return 1;
  if (fuse_stem(m)) return 1;
  if (attach_group_norm_scratch(m)) return 1;
  if (plan_arena(m)) return 1;
  if (upload_conv_records(m)) return 1;
  return 0;
}

}  // namespace odt
