// libodt_hip.so -- host-side model of a handle: the static execution plan (ops, conv records, tensors), its memory
// (weights, activation arena, workspaces, ingest slots) and the helpers shared by the plan builders (plan_common.hip,
// plan_fpn.hip, plan_effdet.hip), the runtime (runtime.hip) and the stand-alone op entry points (op_shims.hpp, op_shims.hip,
// op_shims_conv.hip).
// Host code only; every device kernel lives in the kernel translation units (conv_*.hip, proposals.hip, ...).
#pragma once
#include "../../include/odt.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <set>
#include <string>
#include <type_traits>
#include <vector>

#include "odt_common.hpp"

namespace odt {

std::string& last_error();          // the calling thread's error message (odt_last_error)
int launch_subsample2(const float* in, int B, int H, int W, int C, float* out, int Ho, int Wo,
                      hipStream_t stream);

struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
  int alloc(size_t n) {
    bytes = n;
    if (n == 0) n = 256;
    ODT_HIP(hipMalloc(&p, n));
    return 0;
  }
  void release() { if (p) (void)hipFree(p); p = nullptr; bytes = 0; }
  ~DevBuf() { release(); }
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
};

struct Tensor {      // NHWC device tensor; (h,w) = logical (possibly sliced) dims
  float* d = nullptr;
  int B = 0, H = 0, W = 0, C = 0;   // allocation dims (C = pixel stride)
  int h = 0, w = 0, c = 0;          // logical dims
  size_t elems() const { return (size_t)B * H * W * C; }
};

struct HostTensor {
  std::vector<float> data;
  std::vector<int64_t> shape;
};

struct ConvOp {
  ConvParams p;
  std::string name;
};

enum OpKind { OP_PRE, OP_CONV, OP_POOL, OP_SUB2, OP_PROPOSALS, OP_ROI_HEAD, OP_DETECT, OP_ROI_FINAL,
              OP_ROI_MASK, OP_MASK_SELECT, OP_PRE_RGB, OP_DW, OP_CMEAN, OP_CSCALE, OP_FUSE, OP_EFF_POST, OP_ROI_EFF, OP_SE_GATE,
              OP_SE_GATE_MEAN, OP_WSCALE, OP_MB_EXPAND_DW, OP_RSE_GATE, OP_RSE_APPLY, OP_GCONV, OP_BLOCK, OP_DCONV, OP_GN, OP_GN_ROI,
              OP_RELATION_GEO, OP_RELATION_ATTN, OP_ATT_POOL, OP_ATT_ADD };
struct Op {
  OpKind kind;
  int conv = -1;        // index into convs (OP_BLOCK: the block's conv2, whose record launches conv_block_kernel)
  int gconv = -1;       // OP_GCONV: its index among the plan's grouped convs (profiling events)
  int dconv = -1;       // OP_DCONV: its index among the plan's deformable convs (profiling events)
  int gnorm = -1;       // OP_GN: its index among the plan's GroupNorm layers (profiling events)
  int gnroi = -1;       // OP_GN_ROI: its index among the plan's ROI GroupNorm layers (profiling events)
  int rel = -1;         // OP_RELATION_GEO / OP_RELATION_ATTN: the relation module it belongs to (0: RM_r1, 1: RM_r2; profiling events)
  Tensor in, out;
  DwConvParams dw{};    // OP_DW
  MbExpandDwParams mb{};   // OP_MB_EXPAND_DW
  FuseParams fuse{};    // OP_FUSE
  SeGateParams se{};    // OP_SE_GATE (aux2 = partial-sum scratch)
  ResSeParams rse{};    // OP_RSE_GATE: pool of conv2's output + the SE-ResNet gate
  ResSeApplyParams rsa{};   // OP_RSE_APPLY: gate * conv3 + shortcut, ReLU
  GroupConvParams gc{};    // OP_GCONV: the ResNeXt block's 32-group 3x3 conv2 (conv_group.hip)
  DeformConvParams dc{};   // OP_DCONV: a deformable stage entry's conv2_offset + deformable conv2 (conv_deform.hip)
  GroupNormParams gn{};    // OP_GN: GroupNorm of a conv's output + what that conv's epilogue would have carried (group_norm.hip)
  RoiGroupNormParams gnr{};   // OP_GN_ROI: GroupNorm behind a conv of the 4-conv box head, per ROI (group_norm_roi.hip)
  RelationGeoParams rg{};     // OP_RELATION_GEO: the geometric bias of a relation module (relation.hip)
  RelationAttnParams ra{};    // OP_RELATION_ATTN: its attention, softmax(Q K^T / sqrt(dh) + bias) V per head (relation.hip)
  AttPoolParams ap{};         // OP_ATT_POOL: the 49-position sum of the RoI features in front of fastrcnn/att_trans (att_head.hip)
  AttAddParams aa{};          // OP_ATT_ADD: hidden + relu(att_trans), the tensor fastrcnn/outputs reads (att_head.hip)
  float* aux = nullptr; // OP_CMEAN: means out [B,ldc]; OP_CSCALE / OP_WSCALE: gates in [B,ldc]
  const float* wt0 = nullptr;   // OP_WSCALE: the conv's unscaled weights [Cout][K] (conv = index of the conv whose weights are rebuilt)
  float* aux2 = nullptr;   // OP_CMEAN: partial-sum scratch
  int pad_t = 0, pad_l = 0;   // OP_PRE_RGB
  bool skip = false;          // OP_CONV folded into its producer's epilogue (fuse_rpn_heads): not launched
};

}  // namespace odt

using namespace odt;      // (odt_model is the C ABI's global handle type)

struct odt_model {
  odt_config cfg;
  Knobs knobs;                       // ODT_* overrides: taken at odt_create, retaken at odt_finalize_weights to build the plan
  int device = 0;
  hipStream_t own_stream = nullptr;
  bool finalized = false;
  std::map<std::string, HostTensor> host_w;
  std::vector<std::unique_ptr<DevBuf>> bufs;
  std::map<std::string, Tensor> taps;
  std::vector<ConvOp> convs;
  std::vector<char> conv_fused;      // convs[i] is evaluated inside another conv's kernel (no launch of its own): 1 RPN head, 2 bottleneck conv3, 3 bottleneck conv1 (OP_BLOCK)
  ConvParams* convs_dev = nullptr;   // device copies of conv_recs
  std::vector<ConvParams> conv_recs; // launch records: convs[i] runs as records [conv_rec0[i], + conv_nrec[i]) (batch ranges,
  std::vector<int> conv_rec0, conv_nrec;   // more than one only where a tensor would reach 2 GiB: upload_conv_records)
  int chunked_convs = 0;
  // |max| slots of the tensors the split conv kernels produce (ConvParams::out_amax / in_amax: the fp16x2 kernels scale
  // their A operand by them).  Two groups, cleared at the start of the ops that fill them: [0, kAmaxSlots) for producers in
  // the trunk, [kAmaxSlots, 2 kAmaxSlots) for producers in the tail ops (which may run under the next forward's trunk).
  static constexpr int kAmaxSlots = 512;
  unsigned* amax_dev = nullptr;
  int amax_used[2] = {0, 0};
  unsigned* range_host = nullptr;        // pinned, device-mapped: the |max| records (kRangeSlots words) of the last completed forward
  std::vector<float> range_baseline;     // per slot: the |max| the host last accepted (odt_range_health)
  unsigned* range_host_dev = nullptr;    // ... its device address (amax_rotate_kernel writes it)
  std::vector<std::string> range_slot_name;
  int convs_h2 = 0;                  // convs on the fp16x2 kernels
  int stem_fused = 0;                // conv0 + pool0 run as one kernel (fuse_stem)
  int convs_h2f = 0;                 // ... of them with the following 1x1 conv folded into the kernel (fuse_bottleneck_tails)
  int blocks_fused = 0;              // identity bottlenecks that run as one conv_block_kernel launch (fuse_bottleneck_blocks)
  unsigned* pre_amax = nullptr;      // range slot of the preprocessed frames (OP_PRE records it; conv0 reads it)
  std::vector<Op> ops;
  // geometry
  int Hp = 0, Wp = 0;
  // proposal / head / detection state
  ProposalParams prop{};
  RoiAlignParams roi_head{}, roi_final{}, roi_mask{};
  MaskSelectParams mask_sel{};
  EffPostParams eff_post{};
  RoiAlignParams roi_eff{};
  int eff_filters = 0;
  struct Slot;
  // D2H of the small outputs enqueued behind the forward on the compute stream (odt_submit_ex without the big
  // [M,C,7,7] features): set by odt_submit_ex for the duration of run_plan
  Slot* d2h_slot = nullptr; int d2h_want = 0;
  ConvPolicy policy{};               // conv arithmetic / kernel-family policy of this handle (attach_split_weights)
  int se_blocks = 0;                 // SE-ResNet (odt_config.use_se): bottlenecks that run pool + gate + apply (resnet_se.hip)
  int gconv_ops = 0;                 // ResNeXt (odt_config.block_kind == 2): launches of the 32-group 3x3 conv per forward (conv_group.hip)
  int dconv_ops = 0;                 // odt_config.use_deformable: stage entries that run conv2_offset + the deformable conv2 (conv_deform.hip)
  int gn_ops = 0;                    // odt_config.use_gn: GroupNorm layers, three launches each (group_norm.hip)
  int gn_roi_ops = 0;                // odt_config.use_gn + use_conv_frcnn_head: ROI GroupNorm layers of the box head, one launch each (group_norm_roi.hip)
  int rel_modules = 0;               // odt_config.add_relation_nn: relation modules of the box head (RM_r1, RM_r2), two launches each (relation.hip)
  int att_head = 0;                  // odt_config.use_att_frcnn_head: the box head runs OP_ATT_POOL, fastrcnn/att_trans and OP_ATT_ADD (att_head.hip)
  int att_conv = -1;                 // ... index of fastrcnn/att_trans in convs (profiling: its time is the conv's)
  int mb_fused = 0;                  // EfficientNet: MBConv blocks whose expand + depthwise run as one kernel (effnet_mbconv.hip)
  // tail overlap: the selection / ROIAlign / box-head / NMS kernels of forward i (a few dozen workgroups each,
  // ~2 ms per 8-frame step) run on a side stream under the backbone of forward i+1.  The next forward's FPN stage
  // (the first op that overwrites what the tail reads: P2..P5, the RPN outputs) waits for the previous tail.
  int tail_overlap = -1;             // -1 undecided | 0 off | 1 on (ODT_TAIL_OVERLAP=0 disables; own stream only)
  size_t op_first_fpn = 0, op_tail = 0;
  hipStream_t tail_stream = nullptr, done_stream = nullptr;
  hipEvent_t trunk_done = nullptr, tail_done = nullptr;
  bool tail_pending = false;
  unsigned long long forwards_enqueued = 0;
  int eff_scaled_h = 0, eff_scaled_w = 0;   // EfficientDet: size of the resized frame inside the padded input
  float* final_masks = nullptr;   // [B*per_im, 28, 28] (add_mask)
  std::map<std::string, std::unique_ptr<DevBuf>> rle_bufs;   // odt_mask_rle: device buffers by name, grown on demand
  MaskRleHost rle_host;                                       // ... and the result of its last call
  DetectParams det{};
  Tensor image_pad, frames_dev;
  int src_h = 0, src_w = 0;          // source frame size (== cfg.height/width unless odt_set_source_size)
  DevBuf frames_src;                 // device staging for source frames larger than the plan's input
  float* anchors_dev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  float* final_feat = nullptr;    // [B*per_im, C, 7, 7] packed
  float* final_pooled = nullptr;  // [B*per_im, C]
  size_t frames_bytes = 0;
  // pipelined ingest: two slots
  struct Slot {
    void* pin_in = nullptr; size_t pin_in_bytes = 0;
    void* dev_in = nullptr; size_t dev_in_bytes = 0;
    float *pin_boxes = nullptr, *pin_probs = nullptr, *pin_feats = nullptr, *pin_pooled = nullptr;
    float* pin_masks = nullptr;
    int *pin_labels = nullptr, *pin_valid = nullptr;
    hipEvent_t h2d_done = nullptr, fwd_done = nullptr, d2h_done = nullptr;
    int ticket = -1;            // outstanding ticket or -1
    int ingest_armed = -1;      // ticket number odt_ingest_buffer() handed pin_in out for (-1: none), and its dtype
    int ingest_dtype = 0;
    int want = 0;               // ODT_WANT_* bits of the outstanding ticket
  } slot[2];
  hipStream_t copy_in = nullptr, copy_out = nullptr;
  int next_ticket = 0;
  hipEvent_t wait_before_detect = nullptr;   // D2H of the previous batch must finish before the tail rewrites outputs
  // profiling
  bool profile = false;
  std::vector<hipEvent_t> ev;
  hipEvent_t ev_total[2] = {nullptr, nullptr};
  double prof_conv_ms = 0, prof_conv_flops = 0, prof_total_ms = 0;
  std::vector<double> prof_layer_ms;
  std::vector<hipEvent_t> ev_gconv;  // OP_GCONV i: events [2 i, 2 i + 1]
  double prof_gconv_ms = 0;
  std::vector<hipEvent_t> ev_dconv;  // OP_DCONV i: events [3 i, 3 i + 2] (before, between the two kernels, after)
  double prof_doff_ms = 0, prof_dconv_ms = 0;
  std::vector<hipEvent_t> ev_gn;     // OP_GN i: events [2 i, 2 i + 1]
  double prof_gn_ms = 0;
  std::vector<hipEvent_t> ev_gn_roi; // OP_GN_ROI i: events [2 i, 2 i + 1]
  double prof_gn_roi_ms = 0;
  std::vector<hipEvent_t> ev_rel;    // relation module i: events [4 i, 4 i + 3] (geo before / after, attention before / after)
  double prof_rel_geo_ms[2] = {0, 0}, prof_rel_attn_ms[2] = {0, 0};
  std::vector<hipEvent_t> ev_att;    // the attention branch: events [0, 1] around OP_ATT_POOL, [2, 3] around OP_ATT_ADD
  double prof_att_pool_ms = 0, prof_att_add_ms = 0;
  int prof_forwards = 0;
  int prof_launches = 0;

  // ---- activation arena (odt_config.keep_taps == 0): stage tensors get VIRTUAL addresses while the plan is built
  // (kVirtBase + running offset: never dereferenced), plan_arena() assigns each the lowest arena offset that no tensor
  // with an overlapping live range [first op, last op] occupies and rewrites every pointer of the plan.  Tensors that
  // must keep their contents between forwards (zero borders, zero pad channels, outputs) stay dedicated allocations.
  struct VTensor { size_t bytes = 0, voff = 0, off = 0; int first = 1 << 30, last = -1, region = 0; };
  static constexpr uintptr_t kVirtBase = 0x400000000000ull;
  bool arena_on = false;
  std::set<std::string> transient_taps;     // stage names whose memory is reused within a forward (arena mode)
  std::vector<VTensor> vt;
  size_t vnext = 0;
  float* arena[2] = {nullptr, nullptr};     // 0: trunk (live ranges end before the tail) | 1: read / written by the tail ops
  size_t arena_bytes[2] = {0, 0};
  size_t dedicated_tensor_bytes = 0, virtual_tensor_bytes = 0;
  bool is_virtual(const void* p) const {
    const uintptr_t a = (uintptr_t)p;
    return a >= kVirtBase && a < kVirtBase + vnext;
  }
  int vt_index(const void* p) const {       // the virtual tensor an address falls into
    const size_t o = (size_t)((uintptr_t)p - kVirtBase);
    size_t lo = 0, hi = vt.size();
    while (hi - lo > 1) { const size_t mid = (lo + hi) / 2; if (vt[mid].voff <= o) lo = mid; else hi = mid; }
    return (int)lo;
  }

  float* alloc_f(size_t elems, bool zero) {
    bufs.emplace_back(new DevBuf());
    if (bufs.back()->alloc(elems * sizeof(float))) return nullptr;
    if (zero && hipMemset(bufs.back()->p, 0, elems * sizeof(float)) != hipSuccess) return nullptr;
    return (float*)bufs.back()->p;
  }
};

namespace odt {

// ---- plan_common.hip
int ceil_div(int a, int b);
int make_tensor(odt_model* m, const std::string& name, int B, int H, int W, int C, Tensor* t, bool zero = false);
const HostTensor* find_w(odt_model* m, const std::string& name);
int same_pad(int in, int k, int s, int* out, int* before);
int bn_fold(odt_model* m, const std::string& scope, int c, double eps, bool keras, std::vector<double>* scale,
            std::vector<double>* shift);
int upload_conv(odt_model* m, const std::string& scope, int kh, int kw, int cin, int cout, bool has_bn, const float** wt_out,
                const float** bias_out);
int upload_conv_cat(odt_model* m, const std::string& sa, int cin_a, const std::string& sb, int cin_b, int cout,
                    const float** wt_out, const float** bias_out);
int upload_conv_plain(odt_model* m, const std::string& scope, int kh, int kw, int cin, int cout, bool has_bias, const float** wt_out,
                      const float** bias_out);
int upload_raw(odt_model* m, const std::vector<float>& v, const float** out);
int upload_group_conv(odt_model* m, const std::string& scope, int C, const float** wt_out, const float** bias_out);
int upload_deform_conv(odt_model* m, const std::string& pre, int C, const float** wt_off, const float** b_off, const float** wt);
int upload_se_gate(odt_model* m, const std::string& pre, int ch, const float** w1, const float** b1, const float** w2t,
                   const float** b2);
// One conv layer of a plan.  What the constructor does not take defaults to a dense same-size conv: 1x1, stride 1, no padding,
// an output of the input's logical size at offset 0 with Cout as its pixel stride, no residual, no activation, no tap.
struct ConvSpec {
  std::string name;
  Tensor in;                          // its logical dims (h, w) bound the reads
  int cin, cout;
  const float *wt = nullptr, *bias = nullptr;   // [cout][kh][kw][cin], [cout] on the device
  int kh = 1, kw = 1, stride = 1, dil = 1, pad_t = 0, pad_l = 0;
  int Ho = -1, Wo = -1;               // -1: in.h / in.w
  int oy = 0, ox = 0;                 // the output's offset in a tensor of [Ho + oy, Wo + ox] pixels
  const Tensor* res = nullptr;        // residual, added as res_mode says (ConvParams::res_mode)
  int res_mode = 0;
  int relu = 0;                       // ConvParams::relu: 0 none | 1 ReLU | 2 swish | 3 sigmoid
  int out_ldc = -1;                   // -1: cout
  const Tensor* in2 = nullptr;        // second source, K-concatenated behind the first: its first cin2 channels at every
  int cin2 = 0, in2_stride = 1;       // in2_stride-th pixel
  std::string tap;                    // stage name of the output
  ConvSpec(const std::string& name_, const Tensor& in_, int cin_, int cout_) : name(name_), in(in_), cin(cin_), cout(cout_) {}
};
int add_conv(odt_model* m, const ConvSpec& s, Tensor* out);
int create_side_stream(hipStream_t* s, const Knobs& k);
ConvPolicy resolve_conv_policy(const odt_model* m);
int attach_split_weights(odt_model* m);
int fuse_rpn_heads(odt_model* m);
int fuse_bottleneck_tails(odt_model* m);
int fuse_bottleneck_blocks(odt_model* m);
int fuse_stem(odt_model* m);
int attach_group_norm_scratch(odt_model* m);
void find_overlap_points(odt_model* m);
int plan_arena(odt_model* m);
int upload_conv_records(odt_model* m);
// ---- plan_fpn.hip / plan_effdet.hip
int build_plan(odt_model* m);
int build_plan_effnet(odt_model* m);
// ---- runtime.hip
int run_plan(odt_model* m, const void* frames, int dtype, int on_device, hipStream_t st);

// odt_rle_result view of a mask_rle host result
inline void rle_fill(const MaskRleHost& h, odt_rle_result* r) {
  r->n = h.n; r->height = h.H0; r->width = h.W0;
  r->strings = h.str.data(); r->offsets = h.off.data(); r->lengths = h.len.data();
  r->counts = h.counts.empty() ? nullptr : h.counts.data();
  r->count_offsets = h.coff.data();
}

// every device pointer op `oi` reads or writes, as a mutable reference (plan_arena: liveness, then the rewrite)
template <typename F>
void visit_op_ptrs(odt_model* m, size_t oi, F&& f) {
  Op& op = m->ops[oi];
  if (op.skip) return;
  auto roi = [&](RoiAlignParams& r) {
    for (auto& p : r.feat) f(p);
    f(r.boxes); f(r.out_nhwc); f(r.out_nchw); f(r.pooled);
  };
  f(op.in.d); f(op.out.d);
  switch (op.kind) {
    case OP_PRE: case OP_PRE_RGB: f(m->image_pad.d); break;
    case OP_CONV: { ConvParams& c = m->convs[op.conv].p; f(c.in); f(c.res); f(c.out); f(c.in2); f(c.head_out); f(c.f_res); f(c.f_out); break; }
    // (the block kernel reads x through b_in and as the shortcut f_res; `in` mirrors b_in: conv1's output does not exist)
    case OP_BLOCK: { ConvParams& c = m->convs[op.conv].p; f(c.in); f(c.b_in); f(c.f_res); f(c.f_out); break; }
    case OP_PROPOSALS: for (auto& l : m->prop.lvl) f(l.rpn); f(m->prop.props); break;
    case OP_ROI_HEAD: roi(m->roi_head); break;
    case OP_ROI_FINAL: roi(m->roi_final); break;
    case OP_ROI_MASK: roi(m->roi_mask); break;
    case OP_ROI_EFF: roi(m->roi_eff); break;
    case OP_DETECT: f(m->det.head_out); f(m->det.props); break;
    case OP_MASK_SELECT: f(m->mask_sel.logits); break;
    case OP_DW: f(op.dw.in); f(op.dw.out); for (auto& p : op.dw.lin) f(p); for (auto& p : op.dw.lout) f(p); break;
    case OP_MB_EXPAND_DW: f(op.mb.x); f(op.mb.out); break;
    case OP_RSE_GATE: f(op.rse.t2); f(op.rse.part); f(op.rse.mean); f(op.rse.rvec); f(op.rse.gate); break;
    case OP_RSE_APPLY: f(op.rsa.y); f(op.rsa.sc); f(op.rsa.gate); f(op.rsa.out); break;
    case OP_GCONV: f(op.gc.in); f(op.gc.out); break;
    case OP_DCONV: f(op.dc.in); f(op.dc.off); f(op.dc.out); break;
    // (part / ab / mean / var are dedicated allocations shared by the plan's GroupNorm layers: attach_group_norm_scratch)
    case OP_GN: f(op.gn.x); f(op.gn.res); f(op.gn.out); break;
    case OP_GN_ROI: f(op.gnr.x); f(op.gnr.out); break;      // (mean / var, where kept, are dedicated allocations)
    case OP_RELATION_GEO: f(op.rg.boxes); f(op.rg.bias); break;
    case OP_RELATION_ATTN: f(op.ra.q); f(op.ra.k); f(op.ra.v); f(op.ra.bias); f(op.ra.out); break;
    case OP_ATT_POOL: f(op.ap.x); f(op.ap.out); break;
    case OP_ATT_ADD: f(op.aa.h); f(op.aa.a); f(op.aa.out); break;
    case OP_FUSE: for (auto& p : op.fuse.in) f(p); f(op.fuse.out); break;
    case OP_EFF_POST: for (auto& p : m->eff_post.cls) f(p); for (auto& p : m->eff_post.box) f(p); break;
    case OP_CMEAN: case OP_CSCALE: case OP_SE_GATE: case OP_SE_GATE_MEAN: case OP_WSCALE: case OP_POOL: case OP_SUB2: break;
  }
}

}  // namespace odt
