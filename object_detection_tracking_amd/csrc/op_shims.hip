// Stand-alone op entry points of the C ABI (include/odt.h: odt_op_*) other than the conv ones (op_shims_conv.hip): host
// pointers in and out, each runs exactly the kernels the forward uses -- what the staged parity tests call.  Every device
// buffer of a call lives in a GBufs (op_shims.hpp), and every call checks its guards before it copies results out.
#include <functional>

#include "op_shims.hpp"

using namespace odt;

namespace {

// device copies of the squeeze-excite gate's weights + its scratch as the plan lays them out (OP_SE_GATE_MEAN): mean / r
// start as sentinels, the gate as zeros (pad channels stay 0)
int se_gate_bufs(GBufs& g, SeGateParams& sp, int HW, int B, int ldc, int mid, int se, const float* w1, const float* b1, const float* w2t,
                 const float* b2) {
  std::memset(&sp, 0, sizeof(sp));
  sp.HW = HW; sp.ldc = ldc; sp.mid = mid; sp.se = se;
  return g.alloc("se_w1", (size_t)se * ldc, &sp.w1, -1, w1) || g.alloc("se_b1", (size_t)se, &sp.b1, -1, b1) ||
         g.alloc("se_w2t", (size_t)se * ldc, &sp.w2t, -1, w2t) || g.alloc("se_b2", (size_t)mid, &sp.b2, -1, b2) ||
         g.alloc("se_mean", (size_t)B * ldc, &sp.mean) || g.alloc("se_r", (size_t)B * 256, &sp.r) ||
         g.alloc("se_gate", (size_t)B * ldc, &sp.gate, 0);
}

// the gate from per-split partial sums as the plan runs it (a fused squeeze): fold + reduce + expand
int se_from_parts(GBufs& g, const float* part, int nsplit, int B, int HW, int ldc, int mid, int se, const float* w1,
                  const float* b1, const float* w2t, const float* b2, float** mean, float** gate) {
  ODT_CHECK(w1 && b1 && w2t && b2 && mid >= 1 && mid <= ldc && se >= 1, "squeeze-excite: bad weights / sizes");
  SeGateParams sp;
  if (se_gate_bufs(g, sp, HW, B, ldc, mid, se, w1, b1, w2t, b2)) return 1;
  sp.part = part; sp.nsplit = nsplit;
  if (launch_se_gate_from_parts(sp, B, nullptr)) return 1;
  *mean = sp.mean; *gate = sp.gate;
  return 0;
}

// what odt_op_detections and odt_op_class_nms share: the per-image counts, the per-class NMS workspace and the outputs of a
// detection tail with p.B, p.C (BG included) and p.per_im set
int detect_bufs(GBufs& g, DetectParams& p, const int32_t* nprops) {
  const size_t nc = (size_t)p.B * (p.C - 1), no = (size_t)p.B * p.per_im;
  return g.alloc("nprops", (size_t)p.B, &p.nprops, -1, nprops) || g.alloc("cls_keep", nc * p.per_im, &p.cls_keep) ||
         g.alloc("cls_count", nc, &p.cls_count) || g.alloc("out_boxes", no * 4, &p.out_boxes) || g.alloc("out_probs", no, &p.out_probs) ||
         g.alloc("out_labels", no, &p.out_labels) || g.alloc("out_valid", (size_t)p.B, &p.out_valid);
}
int detect_results(const DetectParams& p, float* boxes, float* probs, int32_t* labels, int32_t* valid) {
  const size_t no = (size_t)p.B * p.per_im;
  if (get_dev(boxes, p.out_boxes, no * 4) || get_dev(probs, p.out_probs, no) || get_dev(labels, p.out_labels, no)) return 1;
  return get_dev(valid, p.out_valid, (size_t)p.B);
}

}  // namespace

extern "C" {

int odt_op_preprocess(int device, const void* frames, int dtype, int B, int H, int W, int pad_t, int pad_l,
                      int Hp, int Wp, float* out) {
  ODT_CHECK(frames && out, "odt_op_preprocess: null argument");
  if (set_dev(device)) return 1;
  const size_t nin = (size_t)B * H * W * 3 * (dtype == ODT_DTYPE_U8 ? 1 : 4), nout = (size_t)B * Hp * Wp * 4;
  GBufs g;
  unsigned char* di;
  float* dout;
  if (g.alloc("frames", nin, &di, -1, frames) || g.alloc("out", nout, &dout)) return 1;
  if (launch_preprocess(di, dtype, B, H, W, pad_t, pad_l, Hp, Wp, dout, nullptr) || g.check("odt_op_preprocess")) return 1;
  return get_dev(out, dout, nout);
}

int odt_op_maxpool(int device, const float* in, int B, int H, int W, int C, float* out) {
  ODT_CHECK(in && out, "odt_op_maxpool: null argument");
  if (set_dev(device)) return 1;
  const int Ho = (H + 1 - 3) / 2 + 1, Wo = (W + 1 - 3) / 2 + 1;
  const size_t nout = (size_t)B * Ho * Wo * C;
  GBufs g;
  float *di, *dout;
  if (g.alloc("in", (size_t)B * H * W * C, &di, -1, in) || g.alloc("out", nout, &dout)) return 1;
  if (launch_maxpool3x3s2(di, B, H, W, C, dout, Ho, Wo, nullptr) || g.check("odt_op_maxpool")) return 1;
  return get_dev(out, dout, nout);
}

int odt_op_topk(int device, const float* scores, int n, int k, int32_t* idx_out) {
  ODT_CHECK(scores && idx_out, "odt_op_topk: null argument");
  if (set_dev(device)) return 1;
  GBufs g;
  float* ds;
  int* di;
  if (g.alloc("scores", (size_t)n, &ds, -1, scores) || g.alloc("idx", (size_t)k, &di)) return 1;
  if (launch_topk(ds, n, k, di, nullptr) || g.check("odt_op_topk")) return 1;
  return get_dev(idx_out, di, (size_t)k);
}

int odt_op_nms(int device, const float* boxes, const float* scores, int n, int max_out, float iou_thresh,
               int32_t* idx_out, int* n_out) {
  ODT_CHECK(idx_out && n_out, "odt_op_nms: null argument");
  if (n == 0) { *n_out = 0; return 0; }
  ODT_CHECK(boxes && scores, "odt_op_nms: null argument");
  if (set_dev(device)) return 1;
  GBufs g;
  float *db, *ds;
  int *di, *dn;
  if (g.alloc("boxes", (size_t)n * 4, &db, -1, boxes) || g.alloc("scores", (size_t)n, &ds, -1, scores) || g.alloc("idx", (size_t)n, &di) ||
      g.alloc("count", (size_t)1, &dn)) return 1;
  if (launch_nms(db, ds, n, max_out, iou_thresh, di, dn, nullptr) || g.check("odt_op_nms")) return 1;
  if (get_dev(n_out, dn, (size_t)1)) return 1;
  return get_dev(idx_out, di, (size_t)*n_out);
}

int odt_op_proposals(int device, int graph, int B, int L, const int* hs, const int* ws, const int* fields,
                     const float* const* rpn, const float* const* anchors, int img_h, int img_w, int K,
                     float nms_thresh, float decode_clip, float* props, int32_t* nprops) {
  ODT_CHECK(L >= 1 && L <= 5 && hs && ws && fields && rpn && anchors && props && nprops, "odt_op_proposals: bad argument");
  if (set_dev(device)) return 1;
  ProposalParams p; std::memset(&p, 0, sizeof(p));
  GBufs g;
  for (int l = 0; l < L; ++l) {
    if (g.alloc("rpn" + std::to_string(l), (size_t)B * hs[l] * ws[l] * kRpnCh, &p.lvl[l].rpn, -1, rpn[l]) ||
        g.alloc("anchors" + std::to_string(l), (size_t)fields[l] * fields[l] * 12, &p.lvl[l].anchors, -1, anchors[l])) return 1;
    p.lvl[l].h = hs[l]; p.lvl[l].w = ws[l]; p.lvl[l].field = fields[l];
  }
  p.nlevels = L; p.graph = graph; p.B = B; p.K = K; p.img_h = img_h; p.img_w = img_w;
  p.nms_thresh = nms_thresh; p.decode_clip = decode_clip;
  const size_t per = (size_t)B * L * K;
  if (g.alloc("cand_boxes", per * 4, &p.cand_boxes) || g.alloc("cand_scores", per, &p.cand_scores) || g.alloc("lvl_boxes", per * 4, &p.lvl_boxes) ||
      g.alloc("lvl_scores", per, &p.lvl_scores) || g.alloc("props", (size_t)B * K * 4, &p.props) || g.alloc("cand_count", (size_t)B * L, &p.cand_count) ||
      g.alloc("lvl_count", (size_t)B * L, &p.lvl_count) || g.alloc("nprops", (size_t)B, &p.nprops) ||
      g.alloc("chunk_keys", (size_t)B * proposal_total_chunks(p) * K, &p.chunk_keys)) return 1;
  if (launch_proposals(p, nullptr) || g.check("odt_op_proposals")) return 1;
  if (get_dev(props, p.props, (size_t)B * K * 4)) return 1;
  return get_dev(nprops, p.nprops, (size_t)B);
}

int odt_op_roi_align(int device, int B, int C, const int* hs, const int* ws, const float* const* feats,
                     const float* strides, const float* boxes, const int32_t* box_ind, int R,
                     float* out_nchw, float* pooled) {
  ODT_CHECK(hs && ws && feats && strides && boxes && box_ind && out_nchw, "odt_op_roi_align: null argument");
  if (R == 0) return 0;
  if (set_dev(device)) return 1;
  RoiAlignParams p; std::memset(&p, 0, sizeof(p));
  GBufs g;
  for (int l = 0; l < 4; ++l) {
    if (g.alloc("feat" + std::to_string(l), (size_t)B * hs[l] * ws[l] * C, &p.feat[l], -1, feats[l])) return 1;
    p.h[l] = p.alloc_h[l] = hs[l]; p.w[l] = p.alloc_w[l] = ws[l]; p.ldc[l] = C;
    p.inv_stride[l] = (float)(1.0 / (double)strides[l]);
  }
  if (g.alloc("boxes", (size_t)R * 4, &p.boxes, -1, boxes) || g.alloc("box_ind", (size_t)R, &p.box_ind, -1, box_ind) ||
      g.alloc("out_nchw", (size_t)R * C * 49, &p.out_nchw)) return 1;
  if (pooled != nullptr && g.alloc("pooled", (size_t)R * C, &p.pooled)) return 1;
  p.C = C; p.per_image = 0; p.count = nullptr; p.R_cap = R;
  if (launch_roi_align(p, nullptr) || g.check("odt_op_roi_align")) return 1;
  if (get_dev(out_nchw, p.out_nchw, (size_t)R * C * 49)) return 1;
  return get_dev(pooled, p.pooled, (size_t)R * C);
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
  for (int l = 0; l < L; ++l) {
    const int32_t* d = dims + 5 * l;
    if (g.alloc("feat" + std::to_string(l), (size_t)B * d[2] * d[3] * d[4], &p.feat[l], -1, feats[l])) return 1;
    p.h[l] = d[0]; p.w[l] = d[1]; p.alloc_h[l] = d[2]; p.alloc_w[l] = d[3]; p.ldc[l] = d[4];
    p.inv_stride[l] = (float)(1.0 / (double)strides[l]);
  }
  if (g.alloc("boxes", (size_t)R * 4, &p.boxes, -1, boxes)) return 1;
  if (count != nullptr && g.alloc("count", (size_t)B, &p.count, -1, count)) return 1;
  if (levels != nullptr && g.alloc("levels", (size_t)R, &p.levels, -1, levels)) return 1;
  if (out_nhwc != nullptr && g.alloc("out_nhwc", (size_t)R * OO * C, &p.out_nhwc)) return 1;
  if (out_nchw != nullptr && g.alloc("out_nchw", (size_t)R * OO * C, &p.out_nchw)) return 1;
  if (pooled != nullptr && g.alloc("pooled", (size_t)R * C, &p.pooled)) return 1;
  if (want_amax && g.alloc("amax", (size_t)1, &p.amax, 0)) return 1;
  p.level0 = level0; p.C = C; p.box_ind = nullptr; p.per_image = per_image; p.R_cap = R; p.out_size = out_size; p.pack_rows = pack_rows;
  if (launch_roi_align(p, nullptr) || g.check("odt_op_roi_align_plan")) return 1;
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
  if (g.alloc("logits", (size_t)R * 14 * 14 * 4 * ld, &p.logits, -1, logits) || g.alloc("labels", (size_t)R, &p.labels, -1, labels) ||
      g.alloc("valid", (size_t)B, &p.valid, -1, valid) || g.alloc("masks", (size_t)R * 784, &p.masks)) return 1;
  p.ld = ld; p.B = B; p.per_image = per_image;
  if (launch_mask_select(p, nullptr) || g.check("odt_op_mask_select")) return 1;
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
  GBufs g;
  DetectParams p; std::memset(&p, 0, sizeof(p));
  p.graph = graph; p.B = B; p.K = K; p.C = C; p.ld = ld; p.img_h = img_h; p.img_w = img_w;
  for (int i = 0; i < 4; ++i) p.reg_w[i] = reg_weights[i];
  p.decode_clip = decode_clip; p.score_thresh = score_thresh; p.nms_thresh = nms_thresh; p.per_im = per_im;
  if (g.alloc("head_out", ho.size(), &p.head_out, -1, ho.data()) || g.alloc("props", (size_t)rows * 4, &p.props, -1, props) ||
      g.alloc("dec_boxes", (size_t)rows * (C - 1) * 4, &p.dec_boxes) || g.alloc("probs", (size_t)rows * C, &p.probs) ||
      detect_bufs(g, p, nprops)) return 1;
  if (launch_detections(p, nullptr) || g.check("odt_op_detections")) return 1;
  return detect_results(p, boxes, probs, labels, valid);
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
  GBufs g;
  DetectParams p; std::memset(&p, 0, sizeof(p));
  p.graph = graph; p.B = B; p.K = N; p.C = Cp;
  p.score_thresh = score_thresh; p.nms_thresh = nms_thresh; p.per_im = per_im;
  if (g.alloc("dec_boxes", (size_t)rows * C * 4, &p.dec_boxes, -1, boxes_in) || g.alloc("probs", pr.size(), &p.probs, -1, pr.data()) ||
      detect_bufs(g, p, ncand)) return 1;
  if (launch_class_nms(p, nullptr) || g.check("odt_op_class_nms")) return 1;
  return detect_results(p, boxes, scores, labels, valid);
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
  if (g.alloc("in", npix_in * ldc, &p.in, -1, in) || g.alloc("wt", (size_t)k * k * ldc, &p.wt, -1, wt) ||
      g.alloc("bias", (size_t)ldc, &p.bias, -1, bias) || g.alloc("out", npix_out * ldc, &p.out)) return 1;
  for (size_t i = 0, off = 0; i < (size_t)nmaps; off += (size_t)p.lH[i] * p.lW[i] * ldc, ++i) {
    p.lin[i] = p.in + off; p.lout[i] = p.out + off;
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
  if (get_dev(out, p.out, npix_out * ldc)) return 1;
  if (squeeze && (get_dev(mean, dmean, (size_t)B * ldc) || get_dev(gate, dgate, (size_t)B * ldc))) return 1;
  return 0;
}

int odt_op_se_gate(int device, const float* x, int B, int HW, int ldc, int mid, int se, const float* w1, const float* b1,
                   const float* w2t, const float* b2, float* mean, float* gate, float* scaled, int32_t* info) {
  ODT_CHECK(x && w1 && b1 && w2t && b2 && mean && gate, "odt_op_se_gate: null argument");
  ODT_CHECK(B >= 1 && HW >= 1 && ldc > 0 && ldc % 4 == 0 && mid >= 1 && mid <= ldc && se >= 1, "odt_op_se_gate: bad sizes");
  if (set_dev(device)) return 1;
  GBufs g;
  SeGateParams sp;
  float *dx, *scratch;
  const int ns = channel_mean_splits(HW, ldc, B);
  if (g.alloc("x", (size_t)B * HW * ldc, &dx, -1, x) || g.alloc("channel_sum scratch", (size_t)B * ns * ldc, &scratch) ||
      se_gate_bufs(g, sp, HW, B, ldc, mid, se, w1, b1, w2t, b2)) return 1;
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
    if (g.alloc("in" + std::to_string(k), (size_t)B * ih * iw * ldc, &p.in[k], -1, ins[k])) return 1;
  }
  if (wsm != nullptr) {      // 'fastattn': relu of the WSM scalars, tf.add_n left to right + 0.0001
    for (int k = 0; k < n; ++k) p.wgt[k] = std::max(wsm[k], 0.f);
    float tot = p.wgt[0];
    for (int k = 1; k < n; ++k) tot = tot + p.wgt[k];
    p.denom = tot + 0.0001f; p.weighted = 1;
  }
  p.n = n; p.act = act; p.B = B; p.h = h; p.w = w; p.ldc = ldc;
  if (g.alloc("out", (size_t)B * h * w * ldc, &p.out)) return 1;
  if (launch_bifpn_fuse(p, nullptr) || g.check("odt_op_bifpn_fuse")) return 1;
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
  float* img;
  ConvParams cp; std::memset(&cp, 0, sizeof(cp));
  if (g.alloc("x", (size_t)B * H * W * in_ldc, &q.x, -1, x) || g.alloc("e_wt", (size_t)mid * in_ldc, &cp.wt, -1, e_wt) ||
      g.alloc("e_bias", (size_t)mid, &q.e_bias, -1, e_bias) || g.alloc("dw_wt", (size_t)k * k * lmid, &q.dw_wt, -1, dw_wt) ||
      g.alloc("dw_bias", (size_t)lmid, &q.dw_bias, -1, dw_bias) ||
      g.alloc("w_img", (mbconv_expand_weight_bytes(lmid, in_ldc) + 3) / 4, &img) ||
      g.alloc("out", (size_t)B * Ho * Wo * lmid, &q.out)) return 1;
  // the expand weights as the bf16x3 piece image of the one-stage 256 x 64 kernel (plan_effdet.hip, fused MBConv)
  cp.Cout = mid; cp.Cin = in_ldc; cp.kh = 1; cp.kw = 1; conv_use_variant(cp, CV_SPLIT1_256x64);
  if (conv_make_split_weights(cp, img, nullptr)) return 1;
  q.B = B; q.H = H; q.W = W; q.in_ldc = in_ldc; q.w_img = img; q.mid = mid; q.lmid = lmid;
  q.Ho = Ho; q.Wo = Wo; q.k = k; q.stride = stride; q.pad_t = pad_t; q.pad_l = pad_l;
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
  return g.alloc("rse_w1", (size_t)r * ch, &gp.w1, -1, w1) || g.alloc("rse_b1", (size_t)r, &gp.b1, -1, b1) ||
         g.alloc("rse_w2t", (size_t)r * cout, &gp.w2t, -1, w2t) || g.alloc("rse_b2", (size_t)cout, &gp.b2, -1, b2) ||
         g.alloc("rse_part", (size_t)B * channel_mean_splits(HW, ch, B) * ch, &gp.part) ||
         g.alloc("rse_mean", (size_t)B * ch, &gp.mean) || g.alloc("rse_rvec", (size_t)B * r, &gp.rvec) ||
         g.alloc("rse_gate", (size_t)B * gp.gate_ld, &gp.gate, 0);
}

}  // namespace

int odt_op_rse_gate(int device, const float* t2, int B, int HW, int ch, int r, int cout, const float* w1, const float* b1,
                    const float* w2t, const float* b2, float* mean, float* gate) {
  ODT_CHECK(t2 && w1 && b1 && w2t && b2 && mean && gate, "odt_op_rse_gate: null argument");
  ODT_CHECK(B >= 1 && HW >= 1 && ch >= 4 && ch % 4 == 0 && r >= 1 && cout >= 1, "odt_op_rse_gate: bad sizes");
  if (set_dev(device)) return 1;
  GBufs g;
  ResSeParams gp;
  if (rse_gate_bufs(g, gp, B, HW, ch, r, cout, w1, b1, w2t, b2) || g.alloc("t2", (size_t)B * HW * ch, &gp.t2, -1, t2)) return 1;
  if (launch_resnet_se_gate(gp, nullptr) || g.check("odt_op_rse_gate")) return 1;
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
  float *dy, *dout;
  // (gate [B, ldc]; out starts as a copy of the caller's buffer: the channels [C, ldc) must come back as they went in)
  if (g.alloc("y", n, &dy, -1, y) || g.alloc("shortcut", n, &ap.sc, -1, shortcut) || g.alloc("gate", (size_t)B * ldc, &ap.gate, -1, gate) ||
      g.alloc("out", n, &dout, -1, out) || alloc_amax(g, &ap.amax)) return 1;
  ap.y = dy; ap.out = in_place ? dy : dout;
  ap.B = B; ap.HW = HW; ap.C = C; ap.ldc = ldc; ap.gate_ld = ldc;
  if (launch_resnet_se_apply(ap, nullptr) || g.check("odt_op_rse_apply") || read_amax(ap.amax, amax)) return 1;
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
  ResSeApplyParams ap; std::memset(&ap, 0, sizeof(ap));
  float *dt2, *dw3, *db3, *dy;
  if (g.alloc("t2", M * ch, &dt2, -1, t2) || g.alloc("w3", w3t.size(), &dw3, -1, w3t.data()) || g.alloc("b3", (size_t)C3, &db3, -1, b3) ||
      g.alloc("shortcut", M * C3, &ap.sc, -1, shortcut) || g.alloc("y", M * C3, &dy) || g.alloc("out", M * C3, &ap.out) ||
      alloc_amax(g, &ap.amax) || rse_gate_bufs(g, gp, B, HW, ch, r, C3, w1, b1, w2t, b2)) return 1;
  gp.t2 = dt2;
  // the plan's order: pool + gate, conv3 (BN folded, no residual, no ReLU), apply
  if (launch_resnet_se_gate(gp, nullptr)) return 1;
  if (run_conv(g, same_conv(dt2, dw3, db3, dy, B, H, W, ch, C3, 1, 1, 0), knobs_read())) return 1;
  ap.y = dy; ap.gate = gp.gate; ap.B = B; ap.HW = HW; ap.C = C3; ap.ldc = C3; ap.gate_ld = gp.gate_ld;
  if (launch_resnet_se_apply(ap, nullptr) || g.check("odt_op_se_tail") || read_amax(ap.amax, amax)) return 1;
  if (get_dev(gate, gp.gate, (size_t)B * C3)) return 1;
  return get_dev(out, ap.out, M * C3);
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
  if (g.alloc("x", nin, &p.in, -1, x) || g.alloc("w", img.size(), &p.wt, -1, img.data()) || g.alloc("bias", (size_t)C, &p.bias, -1, bias) ||
      g.alloc("out", nout, &p.out) || alloc_amax(g, &p.out_amax)) return 1;
  p.B = B; p.H = H; p.W = W; p.C = C; p.Ho = Ho; p.Wo = Wo; p.stride = stride; p.dil = dil; p.pad_t = pad_t; p.pad_l = pad_l;
  p.relu = relu ? 1 : 0;
  if (launch_group_conv(p, nullptr) || g.check("odt_op_group_conv") || read_amax(p.out_amax, amax)) return 1;
  return get_dev(out, p.out, nout);
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
  if (g.alloc("x", nin, &p.in, -1, x) || g.alloc("w_off", io.size(), &p.wt_off, -1, io.data()) || g.alloc("b_off", (size_t)18, &p.b_off, -1, b_off) ||
      g.alloc("w", iw.size(), &p.wt, -1, iw.data()) || g.alloc("offsets", npx * 18, &p.off) || g.alloc("out", npx * C, &p.out) ||
      alloc_amax(g, &p.out_amax)) return 1;
  p.B = B; p.H = H; p.W = W; p.Ha = Ha; p.Wa = Wa; p.ldc = ldc; p.C = C; p.Ho = Ho; p.Wo = Wo;
  if (launch_deform_conv(p, nullptr) || g.check("odt_op_deform_conv") || read_amax(p.out_amax, out_amax)) return 1;
  if (get_dev(offsets_out, p.off, npx * 18)) return 1;
  return get_dev(out, p.out, npx * C);
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
  // (out starts as a copy of the caller's buffer: what lies outside the view must come back as it went in)
  if (g.alloc("x", n, &p.x, -1, x) || g.alloc("gamma", (size_t)C, &p.gamma, -1, gamma) || g.alloc("beta", (size_t)C, &p.beta, -1, beta) ||
      g.alloc("out", n, &p.out, -1, out) || alloc_amax(g, &p.amax) ||
      g.alloc("ab", (size_t)B * 2 * C, &p.ab) || g.alloc("mean", (size_t)B * kGnGroups, &p.mean) || g.alloc("var", (size_t)B * kGnGroups, &p.var)) return 1;
  if (res_mode != 0 && g.alloc("res", (size_t)B * res_H * res_W * C, &p.res, -1, res)) return 1;
  // (the launcher checks chunks against h; an allocation sized from a bad value must not come first)
  const int parts = group_norm_parts(h, w, C, chunks >= 1 && chunks <= h ? chunks : 0);
  if (g.alloc("part", (size_t)B * kGnGroups * parts * 2, &p.part)) return 1;
  p.B = B; p.h = h; p.w = w; p.C = C; p.Ha = Ha; p.Wa = Wa; p.ldc = ldc; p.xoy = oy; p.xox = ox;
  p.oH = Ha; p.oW = Wa; p.out_ldc = ldc; p.oy = oy; p.ox = ox;
  p.res_mode = res_mode; p.res_H = res_H; p.res_W = res_W; p.res_ldc = C; p.relu = relu ? 1 : 0; p.eps = eps; p.chunks = chunks;
  if (launch_group_norm(p, nullptr) || g.check("odt_op_group_norm") || read_amax(p.amax, amax)) return 1;
  if (get_dev(mean, p.mean, (size_t)B * kGnGroups) || get_dev(var, p.var, (size_t)B * kGnGroups)) return 1;
  return get_dev(out, p.out, n);
}

int odt_op_group_norm_roi(int device, const float* x, int R, int h, int w, int ldc, int C, const float* gamma, const float* beta,
                          float eps, float* out, float* amax, float* mean, float* var) {
  ODT_CHECK(x && gamma && beta && out && amax && mean && var, "odt_op_group_norm_roi: null argument");
  ODT_CHECK(R >= 1 && h >= 1 && w >= 1 && ldc >= 1 && C >= 1 && (double)R * h * w * ldc < 1073741824.0, "odt_op_group_norm_roi: bad sizes");
  if (set_dev(device)) return 1;
  GBufs g;
  RoiGroupNormParams p; std::memset(&p, 0, sizeof(p));
  const size_t n = (size_t)R * h * w * ldc;
  // (out starts as a copy of the caller's buffer: the pad channels must come back as they went in)
  if (g.alloc("x", n, &p.x, -1, x) || g.alloc("gamma", (size_t)C, &p.gamma, -1, gamma) || g.alloc("beta", (size_t)C, &p.beta, -1, beta) ||
      g.alloc("out", n, &p.out, -1, out) || alloc_amax(g, &p.amax) ||
      g.alloc("mean", (size_t)R * kGnGroups, &p.mean) || g.alloc("var", (size_t)R * kGnGroups, &p.var)) return 1;
  p.R = R; p.hw = h * w; p.C = C; p.ldc = ldc; p.out_ldc = ldc; p.eps = eps;
  if (launch_group_norm_roi(p, nullptr) || g.check("odt_op_group_norm_roi") || read_amax(p.amax, amax)) return 1;
  if (get_dev(mean, p.mean, (size_t)R * kGnGroups) || get_dev(var, p.var, (size_t)R * kGnGroups)) return 1;
  return get_dev(out, p.out, n);
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
  // (bias starts as a copy of the caller's buffer: what the kernel does not evaluate must come back as it went in)
  if (g.alloc("boxes", (size_t)K * 4, &p.boxes, -1, boxes) || g.alloc("weights", (size_t)kRelGeoWeights, &p.wts, -1, wts) ||
      g.alloc("count", (size_t)1, &p.count, -1, &n) || g.alloc("bias", nb, &p.bias, -1, bias)) return 1;
  p.B = 1; p.K = K; p.Kp = Kp;
  if (launch_relation_geo(p, nullptr) || g.check("odt_op_relation_geo")) return 1;
  return get_dev(bias, p.bias, nb);
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
  if (g.alloc("q", (size_t)K * D, &p.q, -1, q) || g.alloc("k", (size_t)K * D, &p.k, -1, k) || g.alloc("v", (size_t)K * D, &p.v, -1, v) ||
      g.alloc("bias", (size_t)kRelHeads * K * Kp, &p.bias, -1, bias) || g.alloc("count", (size_t)1, &p.count, -1, &n) ||
      g.alloc("out", out_elems, &p.out, -1, out) || alloc_amax(g, &p.amax)) return 1;
  p.B = 1; p.K = K; p.Kp = Kp; p.D = D; p.qk_ldc = D; p.v_ldc = D;
  if (launch_relation_attention(p, nullptr) || g.check("odt_op_relation_attention") || read_amax(p.amax, amax)) return 1;
  return get_dev(out, p.out, out_elems);
}

int odt_op_att_pool(int device, const float* x, int R, int C, float* out, float* amax) {
  ODT_CHECK(x && out && amax, "odt_op_att_pool: null argument");
  ODT_CHECK(R >= 1 && C >= 1 && (double)R * 49 * C < 1073741824.0, "odt_op_att_pool: bad sizes");
  ODT_CHECK(C % 4 == 0, "odt_op_att_pool: C must be a multiple of 4 (C = " + std::to_string(C) + ")");
  if (set_dev(device)) return 1;
  GBufs g;
  AttPoolParams p; std::memset(&p, 0, sizeof(p));
  if (g.alloc("x", (size_t)R * 49 * C, &p.x, -1, x) || g.alloc("out", (size_t)R * C, &p.out) || alloc_amax(g, &p.amax)) return 1;
  p.R = R; p.C = C;
  if (launch_att_pool(p, nullptr) || g.check("odt_op_att_pool") || read_amax(p.amax, amax)) return 1;
  return get_dev(out, p.out, (size_t)R * C);
}

int odt_op_att_add(int device, const float* h, int ldh, const float* a, int R, int D, float* out, float* amax) {
  ODT_CHECK(h && a && out && amax, "odt_op_att_add: null argument");
  ODT_CHECK(R >= 1 && D >= 1 && ldh >= 1 && (double)R * ldh < 1073741824.0 && (double)R * D < 1073741824.0, "odt_op_att_add: bad sizes");
  ODT_CHECK(D % 4 == 0, "odt_op_att_add: D must be a multiple of 4 (D = " + std::to_string(D) + ")");
  ODT_CHECK(ldh >= D && ldh % 4 == 0, "odt_op_att_add: ldh must be a multiple of 4 and at least D (ldh = " + std::to_string(ldh) + ", D = " +
                                          std::to_string(D) + ")");
  if (set_dev(device)) return 1;
  GBufs g;
  AttAddParams p; std::memset(&p, 0, sizeof(p));
  if (g.alloc("h", (size_t)R * ldh, &p.h, -1, h) || g.alloc("a", (size_t)R * D, &p.a, -1, a) || g.alloc("out", (size_t)R * D, &p.out) ||
      alloc_amax(g, &p.amax)) return 1;
  p.R = R; p.D = D; p.ldh = ldh;
  if (launch_att_add(p, nullptr) || g.check("odt_op_att_add") || read_amax(p.amax, amax)) return 1;
  return get_dev(out, p.out, (size_t)R * D);
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
  int tot = 0;
  for (int l = 0; l < 5; ++l) {
    ODT_CHECK(npix[l] >= 1 && cls[l] && box[l], "odt_op_effdet_post: bad level");
    if (g.alloc("cls" + std::to_string(l + 3), (size_t)B * npix[l] * ldc_cls, &p.cls[l], -1, cls[l]) ||
        g.alloc("box" + std::to_string(l + 3), (size_t)B * npix[l] * ldc_box, &p.box[l], -1, box[l])) return 1;
    p.npix[l] = npix[l]; p.anchor_off[l] = tot; tot += npix[l] * 9;
  }
  p.anchor_off[5] = tot;
  p.ldc_cls = ldc_cls; p.ldc_box = ldc_box; p.ncls = ncls; p.B = B; p.k = k; p.max_out = max_out;
  p.score_thresh = score_thresh; p.iou_thresh = iou_thresh; p.image_scale = image_scale;
  const size_t nlog = (size_t)tot * ncls;
  if (g.alloc("anchors", (size_t)tot * 4, &p.anchors, -1, anchors) || g.alloc("keys", nlog, &p.keys) ||
      g.alloc("hist", 256, &p.hist, 0) || g.alloc("state", 5, &p.state, 0) || g.alloc("sel", (size_t)B * k, &p.sel) ||
      g.alloc("cand_boxes", (size_t)B * k * 4, &p.cand_boxes) || g.alloc("cand_scores", (size_t)B * k, &p.cand_scores) ||
      g.alloc("cand_cls", (size_t)B * k, &p.cand_cls) || g.alloc("cand_lvl", (size_t)B * k, &p.cand_lvl) ||
      g.alloc("out_boxes", (size_t)B * max_out * 4, &p.out_boxes) || g.alloc("out_scores", (size_t)B * max_out, &p.out_scores) ||
      g.alloc("out_labels", (size_t)B * max_out, &p.out_labels) || g.alloc("out_levels", (size_t)B * max_out, &p.out_levels) ||
      g.alloc("out_valid", (size_t)B, &p.out_valid)) return 1;
  if (launch_effdet_post(p, nullptr) || g.check("odt_op_effdet_post")) return 1;
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
