// Shared declarations for libodt_hip.so (gfx950).  Kernel launch wrappers are
// declared here and defined in the per-kernel .hip translation units.
#pragma once
#include <hip/hip_runtime.h>
#include <vector>

#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <functional>
#include <string>

#include "knobs.hpp"

namespace odt {

void set_error(const std::string& msg);

#define ODT_HIP(expr)                                                          \
  do {                                                                         \
    hipError_t odt_e_ = (expr);                                                \
    if (odt_e_ != hipSuccess) {                                                \
      ::odt::set_error(std::string(#expr) + ": " + hipGetErrorString(odt_e_)); \
      return 1;                                                                \
    }                                                                          \
  } while (0)

#define ODT_CHECK(cond, msg)                 \
  do {                                       \
    if (!(cond)) {                           \
      ::odt::set_error(std::string(msg));    \
      return 1;                              \
    }                                        \
  } while (0)

typedef float f32x4 __attribute__((vector_size(16)));
typedef float f32x16 __attribute__((vector_size(64)));

constexpr int kMaxTopK = 1024;   // rpn_test_post_nms_topk handled by the one-candidate-per-thread selection kernels
constexpr int kMaxTopKBig = 4096;// rpn_test_post_nms_topk upper bound (above kMaxTopK: the *_big kernels, paneled NMS)
#ifndef ODT_AMAX_WAYS
#define ODT_AMAX_WAYS 1
#endif
// words per tensor range slot (ConvParams::in_amax / out_amax; conv_split_common.hpp amax_read / amax_way).  1: one word per
// tensor.  Round 5 measured 16 (-DODT_AMAX_WAYS=16, tools/ab_build_all.sh: a sixteenth of the same-address atomics when a
// launch's workgroups finish together): b = 8 310.0 -> 308.7 FPS, b = 1 174.0 -> 164.0 (profiles/r05_amax_ways_ab.txt) -- the
// sixteen reads in front of every consumer's first load cost more than the atomics they spare.  Not kept.
constexpr int kAmaxWays = ODT_AMAX_WAYS;
// Round 6 (the continuous fp16x2 range guard): a plan's slot array is [live |max| : kRangeSlots][previous forward's |max| : kRangeSlots];
// amax_rotate_kernel (runtime.hip; the former memset at the start of a forward) moves a group's records to the second row and to
// host-visible memory, where odt_range_health compares them with the values the host last accepted -- no kernel code beyond what
// recorded the maxima all along (counters in the producers were built and cost 1 %: tools/experiments/r06_range_counters).
constexpr int kRangeSlots = 1024;
constexpr int kRoiOut = 7;       // ROIAlign output side (models.py:703)
constexpr int kRpnCh = 16;       // 3 logits + 12 deltas (+1 pad) per pixel
constexpr int kSelChunk = 32768; // logits per workgroup in stage 1 of the RPN top-k
int proposal_total_chunks(const struct ProposalParams& p);

// ---------------------------------------------------------------- conv (K2+K3)
// Implicit-GEMM convolution, NHWC fp32, exact-f32 MFMA (v_mfma_f32_32x32x2_f32).
//   out[n,ho+oy,wo+ox,co] = act( sum_{kh,kw,ci} in[n,ho*s+kh*d-pt, wo*s+kw*d-pl, ci]
//                                * wt[co,kh,kw,ci] + bias[co] (+ residual) )
struct ConvParams {
  const float* in;     // [B,H,W,in_ldc]  (first Cin channels read)
  const float* wt;     // [Cout][kh][kw][Cin]  (K contiguous), BN folded
  const float* bias;   // [Cout]
  const float* res;    // residual (see res_mode) or nullptr
  float* out;          // [B,out_H,out_W,out_ldc]
  int B, H, W, Cin, in_ldc;   // H,W: logical input extent (reads outside are zero)
  int in_Ha, in_Wa;           // allocation extent of `in` (row pitch); >= H,W (sliced views)
  int Ho, Wo, Cout;
  int kh, kw, stride, dil, pad_t, pad_l;
  int out_H, out_W, out_oy, out_ox, out_ldc;
  int res_mode;        // 0 none | 1 same shape | 2 nearest-2x upsample of [B,res_H,res_W,*]
  int res_H, res_W, res_ldc;
  int relu;            // epilogue activation: 0 none | 1 ReLU | 2 swish x*sigmoid(x) | 3 sigmoid
  // optional second A source, K-concatenated behind the first (1x1 convs only): the stage-entry
  // bottleneck computes conv3(t2) + convshortcut(x) as ONE GEMM over [t2 | x(::stride2)]
  const float* in2;    // [B,in2_Ha,in2_Wa,in2_ldc] or nullptr
  int Cin2, in2_ldc, in2_Ha, in2_Wa, in2_stride;
  unsigned div_howo_mul, div_howo_sh, div_wo_mul, div_wo_sh;   // exact m / (Ho*Wo), r / Wo by multiply-shift (conv_prepare)
  int debug;           // ablation bits for kernel tuning (0 in production; ODT_CONV_DEBUG)
  unsigned long long* trace;   // optional [grid][8] wall-clock phase stamps (tuning only)
  // optional bf16-piece image of `wt` (conv_make_split_weights): the layer runs on the bf16x3
  // split kernel (conv_split.hip: f32 result through six exact bf16 MFMA products per MAC)
  const void* wt_split;
  // which kernel instantiation runs this record: a row of the conv kernel table (ConvVariant below; conv_use_variant is the
  // only writer).  HOST-ONLY, like the slots beside it -- of the launch choices the kernels read `splitk` alone.  The row
  // names the family the weight image was laid out for, the block tile bm x bn and the kw-reuse / double-stage / fused
  // forms; 0: none chosen (yet).
  int variant;
  int host_unused0_[3];
  // split-K (the conv_split3 and fp16x2 kernels): the reduction is cut into `splitk` contiguous ranges of stages, one workgroup per
  // (tile, range); each writes its raw f32 partial tile to partial[range][M][Cout] and split_reduce_kernel adds them in
  // range order (deterministic) and applies bias / residual / activation.  For layers whose tiles cannot fill the chip.
  int splitk;          // 0 / 1: off
  float* partial;      // scratch [splitk][M][Cout] (plan-owned, shared by the plan's split-K layers)
  // optional fused 1x1 head behind this conv (conv_split3 kernels whose n-tile is the whole Cout = 256: the RPN 3x3 conv +
  // ReLU, models.py:979-1009): head_out[m][j] = sum_c act(conv)[m][c] * head_wt[c][j] + head_bias[j], j < 16, evaluated on
  // the staged C tile in the epilogue with exact-f32 MFMA (v_mfma_f32_16x16x4_f32) -- the 256-channel tensor is never
  // written (out == nullptr) or read back, and the separate N = 15 launch disappears
  // optional per-row-range epilogue constants (conv_split3 kernels without split-K): rows [lvl_start[i], lvl_start[i+1])
  // of the GEMM take bias[i * lvl_stride + c] and, if given, the factor lvl_scale[i * lvl_stride + c] in front of it
  // (out = act(acc * scale + bias)).  The EfficientDet class / box nets share their conv weights between the five pyramid
  // levels but carry one BatchNorm per level (efficientdet_arch.py:227-393): with the levels' pixels concatenated (each
  // padded to whole 256-row tiles) a layer is ONE launch instead of five.
  int nlvl;            // 0 / 1: off
  int lvl_start[5];
  int lvl_stride;
  const float* lvl_scale;
  // fp16x2 pieces (CF_H2 rows, conv_h2.hip): the A operand is scaled by a power of two taken from the recorded |max|
  // of the source tensor(s) -- a u32 holding the f32 bit pattern, written by the producers' epilogues (out_amax: atomic max
  // over the stored values; the plan clears the slots at the start of a forward) -- and the weight image's column n by
  // 2^t_n; the epilogue multiplies the accumulators by h2_chinv[n] = 2^-t_n and by the inverse of the A scale.
  const unsigned* in_amax;   // |max| of `in` (required for the CF_H2 rows)
  const unsigned* in2_amax;  // ... of `in2`
  unsigned* out_amax;        // where this conv records the |max| of what it stores (any split kernel), or nullptr
  const float* h2_chinv;     // [cout_padded(Cout)] (CF_H2 rows)
  const float* head_wt;    // [Cout][16] (k-major, column 15 zero) or nullptr
  const float* head_bias;  // [16]
  float* head_out;         // [M][head_ldc] dense rows (m = (n, ho, wo))
  int head_ldc;
  // optional fused 1x1 conv behind this conv (conv_h2k_kernel<.., FUSE>: the bottleneck's conv2 3x3 + BN + ReLU followed by
  // conv3 1x1 + BN (+ shortcut) + ReLU, nn.py:503-521): the tile's accumulators never leave the CU -- scaled, biased and
  // activated in registers, split into fp16x2 pieces with a power of two PER PIXEL ROW (not per tensor), they are the
  // second GEMM's operand as they sit (MFMA C layout == operand layout under a k permutation that the weight image
  // f_wt carries); f_out[m][n] = act(sum_k y[m][k] w[n][k] + f_bias[n] (+ f_res[m][n])), rows m dense over (n, ho, wo).
  // `out` is not written (nullptr) and the 1x1 conv's own launch disappears.
  const void* f_wt;        // conv_make_h2f_weights image of the 1x1 conv (K = this conv's Cout), or nullptr
  const float* f_chinv;    // [f_cout] inverse powers of two of the image's rows
  const float* f_bias;     // [f_cout]
  const float* f_res;      // [M][f_res_ldc] same-shape residual or nullptr
  float* f_out;            // [M][f_out_ldc]
  unsigned* f_out_amax;    // range slot of f_out or nullptr
  int f_cout, f_out_ldc, f_res_ldc, f_relu;
  int host_unused1_[5];
  int reduce_blocks;   // block cap of the split-K combine pass (ODT_SPLIT_REDUCE_BLOCKS; conv_select)
  // optional 1x1 conv IN FRONT of this 3x3 conv + fused tail (conv_block.hip: conv_block_kernel, the whole identity bottleneck
  // out = relu(conv3(relu(conv2(relu(conv1(x))))) + x) in one launch; OP_BLOCK, fuse_bottleneck_blocks): conv1's output lives
  // as an 18 x 18 pixel patch of fp16x2 pieces in LDS, `in` is never read.  Behind every field the other kernels know.
  const float* b_in;         // x: [B,H,W,b_in_ldc], conv1's input (and, as f_res, the block's shortcut), or nullptr
  const void* b_wt;          // conv1's weight image (conv_make_h2_weights, 64-wide n-tile)
  const void* b_wt2;         // this conv's weight image with k in the patch's order (conv_make_h2p_weights)
  const float* b_chinv;      // [64] conv1's inverse column powers of two
  const float* b_bias;       // [64] conv1's bias
  const unsigned* b_in_amax; // range slot of x
  int b_cin, b_in_ldc;
};
// the device record does not move when a host-only slot changes its meaning (tests/test_kernel_resources.py: one awkward
// field once pushed the kernels' copy of it into scratch)
static_assert(sizeof(ConvParams) == 488 && offsetof(ConvParams, variant) == 208 && offsetof(ConvParams, splitk) == 224 &&
              offsetof(ConvParams, nlvl) == 240 && offsetof(ConvParams, reduce_blocks) == 428 && offsetof(ConvParams, b_in) == 432,
              "ConvParams layout");
// fills the derived fields (multiply-shift divisors)
void conv_prepare(ConvParams& p);
double conv_flops(const ConvParams& p);   // algorithmic 2*M*N*K

// ---- the conv kernel table (conv_split.hip owns the lookup; each family file contributes its rows and launch thunks) ----
// One row per kernel instantiation a conv record can run on.  Selection (conv_select), validation (conv_check) and the
// one launcher (launch_conv) all read this table; nothing else knows which (tile, form) combinations exist.
enum ConvFamily : int { CF_F32 = 0, CF_SPLIT1 = 1, CF_H2 = 2, CF_SPLIT3 = 3 };   // exact f32 | one-stage bf16x3 | fp16x2 | 8-wave bf16x3
// (the split families' values are also the layout ids of their weight images: conv_make_split_weights)
enum ConvVariantFlag : unsigned {
  CVF_KWR = 1u,      // kw-reuse kernel: the three kw taps of a (slice, kh) group share one staged run of pixels
  CVF_DSTAGE = 2u,   // conv_h2d_kernel: double stages for the dense 1x1 reductions on two-wave tiles
  CVF_FTAIL = 4u,    // conv_h2k_kernel<.., FUSE>: the bottleneck's conv3 evaluated from conv2's accumulators (ConvParams::f_wt)
  CVF_STEM = 8u,     // conv_stem_kernel: conv0 + pool0, persistent workgroups; `out` is the 3x3 / stride-2 max-pooled map
                     // [B, out_H, out_W, out_ldc] of the conv's [B, Ho, Wo, Cout] result, which is not written
  CVF_ST2 = 16u,     // exact f32: two LDS stages
  CVF_FINE = 32u,    // exact f32: fine-grained loop
};
#define ODT_CONV_VARIANT_LIST(X)                                                                                                   \
  X(F32_128x64_S1) X(F32_128x64_S1_FINE) X(F32_128x64_S2) X(F32_128x64_S2_FINE) X(F32_64x64_S1) X(F32_64x64_S1_FINE)              \
  X(F32_64x64_S2) X(F32_64x64_S2_FINE) X(F32_128x128_S1) X(F32_128x128_S1_FINE) X(F32_128x128_S2) X(F32_128x128_S2_FINE)          \
  X(SPLIT1_128x256) X(SPLIT1_256x128) X(SPLIT1_256x64)                                                                            \
  X(SPLIT3_256x256) X(SPLIT3_256x128) X(SPLIT3_256x64) X(SPLIT3_128x256) X(SPLIT3_128x128)                                        \
  X(SPLIT3K_256x256) X(SPLIT3K_256x128) X(SPLIT3K_256x64)                                                                         \
  X(H2_64x64) X(H2_64x128) X(H2_512x64) X(H2_128x64) X(H2_256x256) X(H2_256x128) X(H2_128x128) X(H2D_64x64) X(H2D_64x128)         \
  X(H2K_256x256) X(H2K_256x128) X(H2K_512x64) X(H2K_256x64) X(H2KF_256x64) X(H2KF_256x128) X(H2KF_256x256) X(H2_STEM)
enum ConvVariant : int {
  CV_NONE = 0,
#define ODT_CONV_VARIANT_ENUM(n) CV_##n,
  ODT_CONV_VARIANT_LIST(ODT_CONV_VARIANT_ENUM)
#undef ODT_CONV_VARIANT_ENUM
  CV_COUNT
};
typedef void (*ConvLaunchFn)(const ConvParams* dev, unsigned grid, hipStream_t stream);
struct ConvKernelRow {
  const char* name;              // stable: tests/golden/conv_choice.json and the tools name rows by it
  int family;                    // ConvFamily
  int bm, bn, threads;           // block tile, threads per workgroup
  unsigned flags;                // ConvVariantFlag
  ConvLaunchFn launch;
  ConvLaunchFn launch_traced;    // the TRACE = true twin, or nullptr: a trace request keeps running `launch`
};
// a family file's row of the conv kernel table (odt_common.hpp: ConvKernelRow) with its launch thunk(s); kernels are passed in
// parentheses, as to hipLaunchKernelGGL
#define ODT_CONV_THUNK(threads, kern) \
  [](const ConvParams* dev, unsigned grid, hipStream_t st) { hipLaunchKernelGGL(kern, dim3(grid), dim3(threads), 0, st, dev); }
#define ODT_CONV_ROW(t, id, fam, bm, bn, threads, flags, kern) \
  t[CV_##id] = ConvKernelRow{#id, fam, bm, bn, threads, flags, ODT_CONV_THUNK(threads, kern), nullptr}
#define ODT_CONV_ROW_T(t, id, fam, bm, bn, threads, flags, kern, kern_traced) \
  t[CV_##id] = ConvKernelRow{#id, fam, bm, bn, threads, flags, ODT_CONV_THUNK(threads, kern), ODT_CONV_THUNK(threads, kern_traced)}
const ConvKernelRow& conv_variant_row(int variant);      // (CV_NONE / out of range: an empty row, launch == nullptr)
// the row of a (family, tile, form), CV_NONE if the table has none
int conv_variant_find(int family, int bm, int bn, unsigned flags);
// the fused-tail row that runs a kw-reuse fp16x2 record's weight image (512 x 64 tiles: the 256-row form), CV_NONE if none
int conv_variant_fused_tail(int variant);
// sets a record's variant by hand (the fusions, the stand-alone op entry points); validated like any other by conv_check
void conv_use_variant(ConvParams& p, int variant, int splitk = 1, int reduce_blocks = 0);
// each family file's rows (conv_igemm.hip, conv_split1.hip, conv_split3.hip, conv_h2.hip, conv_h2d.hip, conv_h2k.hip, conv_stem.hip)
void conv_rows_f32(ConvKernelRow* t);
void conv_rows_split1(ConvKernelRow* t);
void conv_rows_split3(ConvKernelRow* t);
void conv_rows_h2(ConvKernelRow* t);
void conv_rows_h2d(ConvKernelRow* t);
void conv_rows_h2k(ConvKernelRow* t);
void conv_rows_stem(ConvKernelRow* t);

// bf16x3 split path (conv_split.hip).  ConvPolicy: which convs take it and which kernel family -- per handle, fixed at
// plan build from odt_config and the handle's ODT_CONV_* overrides (conv_policy_with_knobs); a stand-alone conv call
// resolves it under the call's knobs.
struct ConvPolicy {
  int arith;            // 0 exact-f32 MFMA everywhere | 1 bf16x3 split kernels where they pay
  int family;           // split kernel families allowed: 1 one-stage only | 3 + conv_split3_kernel where it fits | 2 + the
                        // fp16x2 kernels (conv_h2.hip) where a layer has 256-row tiles and a recorded input range
  long min_tiles;       // tiles a layer must offer the one- / two-stage kernels (256)
  long min_tiles3;      // ... conv_split3_kernel's 256- / 128-row tiles (200)
  int min_k, min_bn;    // shortest reduction / narrowest n-tile taken
  int h2s_maxk;         // fp16x2: longest reduction that takes the 128 x 128 4-wave tile (two workgroups per CU); 0: none
  bool h2_few_tiles;    // fp16x2: 128 x 128 tiles for the layers without enough 256-row tiles
  bool h2_n64;          // fp16x2: also the 64-wide layers (128 x 64 tiles on 4 waves; the kw-reuse kernel's 256 x 64 tile)
  bool h2k_splitk;      // fp16x2: kw-reuse kernel + split-K over (slice, kh) groups for the KH x 3 layers of few rows
  int h2k_fewrows;      // fp16x2: 1 = kw-reuse kernel on 256 x 128 tiles without split-K where those alone fill the chip; 2 (A/B): the dense 1x1 layers too
  int fill_div;         // a split-K layer is taken when tiles x ranges >= min_tiles3 / fill_div (6)
  int h2_bm64;          // fp16x2: 64 x 128 two-wave tiles for the layers of few rows: 0 off | 1 K <= 1024, no split-K | 2 + longer K cut in two | 3 = 1 on 64 x 64 tiles
  int h2_n64_bm512;     // fp16x2 kw-reuse kernel on 64-wide layers: 512 x 64 tiles -- 0 off | 1 where they fill the chip | 2 wherever valid
  int force_bm3;        // 0 auto | 128 | 256: force conv_split3_kernel with that tile height (tests)
  int splitk_max;       // conv_split3_kernel: largest split-K factor the policy may choose (1 = off)
  bool kw_reuse;        // conv_split3k_kernel for the stride-1 KH x 3 layers it fits (ODT_CONV_SPLIT3_KWR=0: off)
  bool kwr_n64;         // ... also for 64-wide layers (256 x 64 tile, wave tile 64 x 32)
  int force_splitk;     // 0 auto | k: force that split-K factor wherever conv_split3_kernel runs (tests)
  bool src2, res2;      // take the K-concatenated stage-entry convs / the 2x-upsampled-residual FPN laterals
};
ConvPolicy conv_policy_default();
ConvPolicy conv_policy_with_knobs(ConvPolicy q, const Knobs& k);
bool conv_split_supported(const ConvParams& p);
// THE selection: which row runs this conv under this policy and these knobs.  Pure: reads the shape fields of p and whether
// its sources come with a recorded range (in_amax / in2_amax), nothing else.  A CF_F32 row = the exact-f32 kernel; a split
// row names the weight-image layout (family, bn) that conv_make_split_weights must build before the launch.
struct ConvChoice {
  int variant, splitk, reduce_blocks;
};
ConvChoice conv_select(const ConvParams& p, const ConvPolicy& q, const Knobs& k);
// finishes a record: conv_prepare, the ODT_CONV_DEBUG bits, the exact-f32 row where no split image is attached (it
// depends on the rows of THIS record -- a plan cuts large convs into batch ranges), then conv_check; once per record, before
// it is copied to the device (the plan's upload_conv_records, the stand-alone conv calls)
int conv_finish(ConvParams& p, const Knobs& k);
int conv_check(const ConvParams& p);      // the launch preconditions of a record: shape, 32-bit offsets (conv_igemm.hip), then ...
int conv_check_variant(const ConvParams& p);      // ... its row of the table against the shape (conv_split.hip)
// THE launcher of a finished, checked record: grid and split-K combine pass from its row; dev: its device copy (the kernels
// read their parameters from there)
int launch_conv(const ConvParams& p, const ConvParams* dev, hipStream_t stream);
// shape predicates shared by selection and validation (each exists once)
bool conv_kwr_fits(const ConvParams& p);           // the kw-reuse kernels: stride-1 KH x 3 convs over rows of the output's pitch
bool conv_h2_sources_ok(const ConvParams& p);      // fp16x2 allowed for this layer: recorded range(s), 32-channel slices
bool conv_h2d_fits(const ConvParams& p);           // conv_h2d.hip: dense same-size 1x1 with at least two double stages
bool conv_stem_fits(const ConvParams& p);          // conv_stem.hip: the plan's conv0 on 64-wide fp16x2 tiles
// THE record rewrite behind conv_stem_fits (the plan's fuse_stem, odt_op_stem): p writes the pooled map and runs CV_H2_STEM
void conv_stem_fuse(ConvParams& p, float* pooled, int H, int W, int ldc);
int conv_stem_grid(const ConvParams& p, unsigned* grid);   // one persistent workgroup per CU of the current device
int conv_k(const ConvParams& p);   // the GEMM's reduction length: kh * kw * Cin (+ Cin2)
size_t conv_split_weight_bytes(int Cout, int K);
int conv_split_bn(int Cout);   // n-tile width of the split configuration for this Cout (0: none)
int conv_split_bm(int Cout);
// builds the weight image of p.wt in the layout of p's row (conv_use_variant first)
// wt_src: source weights if not p.wt; kscale[K]: per-k factor folded into the weights first (single-source 1x1 convs: a
// per-input-channel gate, e.g. squeeze-excite, applied to the weights instead of the activations)
int conv_make_split_weights(const ConvParams& p, void* img_dev, hipStream_t stream, const float* wt_src = nullptr,
                            const float* kscale = nullptr);
int conv_scale_weights(const float* wt, const float* kscale, int Cout, int K, float* out, hipStream_t stream);
// points p at its finished image: wt_split and, for the CF_H2 rows, h2_chinv (behind the pieces of p's own Cout x conv_k)
void conv_attach_weights(ConvParams& p, const void* img);
// fp16x2 pieces (conv_h2.hip; CF_H2 rows): the image (conv_make_split_weights builds it) carries the per-column
// inverse scales behind the pieces -- ConvParams::h2_chinv must point there; launch_tensor_amax records the |max| of a dense
// array for a source tensor no producer recorded one for (stand-alone calls)
const float* conv_h2_chinv(const void* img, int Cout, int K);
int conv_make_h2_weights(const ConvParams& p, void* img_dev, hipStream_t stream);
int launch_tensor_amax(const float* x, size_t n, unsigned* slot, hipStream_t stream);
// fused 1x1 conv behind a conv_h2k launch (ConvParams::f_wt): image of wt [Cout][K] (K = 128 or 256: the producer's
// Cout), chunks of 32 output columns, k in the order the producer's accumulator registers hold it; the rows' inverse
// powers of two sit behind the pieces (conv_h2f_chinv)
size_t conv_h2f_weight_bytes(int Cout, int K);
const float* conv_h2f_chinv(const void* img, int Cout, int K);
int conv_make_h2f_weights(const float* wt, int Cout, int K, void* img_dev, hipStream_t stream);
bool conv_h2f_fusable(const ConvParams& a, const ConvParams& b);   // a: the KH x 3 producer, b: the 1x1 conv reading a.out
// THE record rewrite behind conv_h2f_fusable (the plan's fuse_bottleneck_tails, odt_op_bottleneck_tail / _block): a becomes the
// fused record -- the fused-tail row of its own image (split-K choices kept), every f_* field from b and b's image `img_f`
// (conv_make_h2f_weights), the residual's non-temporal bit (debug & 0x400) with it; a's own output and range slot are gone
void conv_h2f_fuse(ConvParams& a, const ConvParams& b, const void* img_f);
// whole identity bottleneck in one kernel (conv_block.hip): a 64-wide 3x3 conv's image with k in the order conv1's accumulator
// registers hold it (same size and row scales as conv_make_h2_weights'), the shape test, the launcher of an OP_BLOCK record
int conv_make_h2p_weights(const ConvParams& p, void* img_dev, hipStream_t stream);
bool conv_block_fits(const ConvParams& c1, const ConvParams& c2);    // c1: the 1x1 conv in front, c2: the 3x3 conv carrying the fused tail
// THE record rewrite behind conv_block_fits (the plan's fuse_bottleneck_blocks, odt_op_bottleneck_block): the b_* fields from c1
// and c2's patch-order image `img_p` (conv_make_h2p_weights); c2 reads c1's input and range, and walks K as c1 did (debug & 0x100)
void conv_block_fuse(ConvParams& c2, const ConvParams& c1, const void* img_p);
int launch_bottleneck_block(const ConvParams& p, const ConvParams* dev, hipStream_t stream);
size_t conv_split_partial_bytes(const ConvParams& p);   // scratch a split-K conv needs (0: none)

// ------------------------------------------------------------ elementwise (K1,K4)
// (amax: optional range slot of the output tensor -- the |max| of what is written goes there, see ConvParams::in_amax)
int launch_preprocess(const void* frames, int dtype, int B, int H, int W, int pad_t, int pad_l,
                      int Hp, int Wp, float* out, hipStream_t stream, unsigned* amax = nullptr);
int launch_preprocess_resize(const void* frames, int dtype, int B, int Hs, int Ws, int H, int W, int pad_t,
                             int pad_l, int Hp, int Wp, float* out, hipStream_t stream, unsigned* amax = nullptr);
int launch_maxpool3x3s2(const float* in, int B, int H, int W, int C, float* out, int Ho, int Wo,
                        hipStream_t stream);

// ------------------------------------------------------- EfficientNet blocks (effnet.hip)
struct DwConvParams {
  const float* in;     // [B,H,W,ldc]
  const float* wt;     // [k*k][ldc]  (BN scale folded, pad channels zero)
  const float* bias;   // [ldc]
  float* out;          // [B,Ho,Wo,ldc]
  int B, H, W, Ho, Wo, ldc, k, stride, pad_t, pad_l;
  int act;             // 0 none | 2 swish
  // optional fused squeeze (MBConv): per-workgroup sums of the OUTPUT per (image, channel) for the squeeze-excite gate,
  // sum_part[b][split][c] (fixed order); channel_mean_fold_kernel (launch_se_gate_from_parts) adds the splits
  float* sum_part;     // [B][nsplit][ldc] or nullptr
  int cqn, nsplit;     // filled by dwconv_plan: channel quads per workgroup (16), pixel splits
  int xcd_bands;       // filled by dwconv_plan: 1 = contiguous band of workgroups per XCD (halo rows shared in its L2)
  // optional: several independent [H,W] maps in one launch (batch 1, stride 1 'SAME': the five pyramid levels of a class /
  // box net layer): map i reads lin[i] and writes lout[i], both [lH[i], lW[i], ldc]; grid z = map
  int nlvl;            // 0: off
  const float* lin[5];
  float* lout[5];
  int lH[5], lW[5];
  int px;              // filled by dwconv_plan: outputs per thread along x (the kernel variant)
};
// fills cqn / nsplit / px / xcd_bands (squeeze: sum_part will be set -- sized [B][nsplit][ldc]) and checks the geometry;
// multi-map records take the largest map's extent
int dwconv_plan(DwConvParams& p, bool squeeze, const Knobs& k);
int launch_dwconv(const DwConvParams& p, hipStream_t stream);
// MBConv front half in one kernel (effnet_mbconv.hip): expand 1x1 + BN + swish -> depthwise k x k + BN + swish (+ squeeze
// partial sums); the expanded tensor stays in LDS
struct MbExpandDwParams {
  const float* x;        // block input [B,H,W,in_ldc]; K of the expand GEMM = in_ldc (pad channels: zero weights)
  int B, H, W, in_ldc;
  const void* w_img;     // bf16x3 piece image of the expand weights [lmid][in_ldc] (conv_make_split_weights, the SPLIT1_256x64 row's layout)
  const float* e_bias;   // [mid] folded BN shift of the expand conv
  int mid, lmid;         // expanded channels, their stride (multiple of 64)
  const float* dw_wt;    // [k*k][lmid]  (BN scale folded, pad channels zero)
  const float* dw_bias;  // [lmid]
  float* out;            // [B,Ho,Wo,lmid]
  int Ho, Wo, k, stride, pad_t, pad_l;
  float* sum_part;       // [B][nsplit][lmid] per-workgroup sums of the output (squeeze-excite), or nullptr
  int nsplit;            // tile ranges per image (0: launch_mbconv_expand_dw picks mbconv_expand_dw_splits())
  int tiles_y, tiles_x;  // filled by the launcher
};
int launch_mbconv_expand_dw(const MbExpandDwParams& p, hipStream_t stream);
int mbconv_expand_dw_splits(const MbExpandDwParams& p);
size_t mbconv_expand_weight_bytes(int lmid, int in_ldc);
struct FuseParams {
  const float* in[3];
  int ih[3], iw[3], mode[3];     // mode 0 same size | 1 nearest resize | 2 max-pool 3x3 s2 'SAME'
  float sy[3], sx[3];            // mode 1: in / out size ratios
  int pt[3], pl[3];              // mode 2: 'SAME' pads before
  float wgt[3], denom;           // weighted: relu(WSM_i), sum + 1e-4
  int n, weighted, act;          // act 0 none | 2 swish
  int B, h, w, ldc;
  float* out;
};
int launch_bifpn_fuse(const FuseParams& p, hipStream_t stream);
int launch_preprocess_rgb(const void* frames, int dtype, int B, int H, int W, int pad_t, int pad_l, int Hp, int Wp,
                          float* out, hipStream_t stream);
int channel_mean_splits(int HW, int ldc, int B);
int launch_preprocess_rgb_resize(const void* frames, int dtype, int B, int Hs, int Ws, int Hr, int Wr, int pad_t,
                                 int pad_l, int Hp, int Wp, float* out, hipStream_t stream);
int launch_channel_mean(const float* in, int B, int HW, int ldc, float* scratch, float* out, hipStream_t stream);
int launch_channel_scale(float* x, const float* s, int B, int HW, int ldc, hipStream_t stream);
struct SeGateParams {
  const float* part; int nsplit;      // filled by launch_se_gate (launch_se_gate_from_parts: by the caller)
  int HW, ldc, mid, se;
  const float* w1;   // [se][ldc]   reduce weights (pad channels zero)
  const float* b1;   // [se]
  const float* w2t;  // [se][ldc]   expand weights, transposed
  const float* b2;   // [mid]
  float* gate;       // [B][ldc]    (pad channels stay 0)
  float* r;          // [B][256]    reduced vector (scratch)
  float* mean;       // [B][ldc]    spatial mean (scratch)
};
int launch_se_gate(const float* in, const SeGateParams& p, int B, float* scratch, hipStream_t stream);
// the gate from the depthwise kernel's fused partial sums (p.part / p.nsplit set by the caller): fold + reduce + expand
int launch_se_gate_from_parts(const SeGateParams& p, int B, hipStream_t stream);

// ------------------------------------------------------- SE-ResNet bottleneck (resnet_se.hip; reference nn.py:506-517)
// gate[b, :] = sigmoid(relu(mean_HW(t2)[b, :] . w1 + b1) . w2 + b2) with conv3 + BN folded into w1 / b1 on the host (the
// spatial mean commutes with the 1x1 conv and the affine BN), then out = max(y * gate[b, c] + shortcut, 0).
struct ResSeParams {
  const float* t2;     // [B,HW,ch] conv2's output (dense)
  int B, HW, ch, r, cout;   // r = ch / 4 reduced channels, cout = 4 ch
  const float* w1;     // [r][ch]    (conv3 . bnscale) @ fc1/W, transposed
  const float* b1;     // [r]        bnshift @ fc1/W + fc1/b
  const float* w2t;    // [r][cout]  fc2/W
  const float* b2;     // [cout]
  float* part;         // scratch [B][channel_mean_splits(HW, ch, B)][ch]
  float* mean;         // [B][ch]
  float* rvec;         // [B][r]
  float* gate;         // [B][gate_ld]
  int gate_ld;         // row stride of gate (>= cout, multiple of 4)
};
int launch_resnet_se_gate(const ResSeParams& p, hipStream_t stream);
// the gate MLP alone, from p.mean
int launch_resnet_se_mlp(const ResSeParams& p, hipStream_t stream);
struct ResSeApplyParams {
  const float* y;      // [B,HW,ldc] conv3 + BN
  const float* sc;     // [B,HW,ldc] shortcut
  const float* gate;   // [B][gate_ld]
  float* out;          // [B,HW,ldc]; may be y.  Channels [C, ldc) are never written
  unsigned* amax;      // range slot of out (|max| of what is stored) or nullptr
  int B, HW, C, ldc, gate_ld;   // ldc, gate_ld multiples of 4
};
int launch_resnet_se_apply(const ResSeApplyParams& p, hipStream_t stream);

// ------------------------------------------------------- 32-group 3x3 conv (conv_group.hip; ResNeXt-32x4d, reference nn.py:524-549)
// out = act(bias + grouped 3x3 conv of in), dense NHWC f32, C = Cin = Cout in {128, 256, 512, 1024}, G = C / 32 channels per
// group; taps outside H x W are zero; plain f32 in a fixed order in every arithmetic mode.
struct GroupConvParams {
  const float* in;     // [B,H,W,C]
  const float* wt;     // group_conv_pack_weights image (BN scale folded)
  const float* bias;   // [C]
  float* out;          // [B,Ho,Wo,C]
  unsigned* out_amax;  // range slot of out (|max| of what is stored) or nullptr
  int B, H, W, C, Ho, Wo, stride, dil, pad_t, pad_l, relu;
};
size_t group_conv_weight_elems(int C);
// hwio [3][3][C / 32][C] times scale[o] (nullptr: 1) in double, rounded once -> dst[group_conv_weight_elems(C)] (host memory)
int group_conv_pack_weights(const float* hwio, const double* scale, int C, float* dst);
int launch_group_conv(const GroupConvParams& p, hipStream_t stream);

// ------------------------------------------------------- deformable 3x3 conv (conv_deform.hip; --use_deformable, reference nn.py:469-485)
// off = conv2_offset(in) at the even positions (3x3, stride 2, one zero row / column in front, + bias), then out = the 3x3
// stride-2 conv of in whose nine taps are bilinear samples at (tap position + off), coordinates clamped to the map.  in is a
// pitched NHWC view; off and out are dense.  Plain f32 in a fixed order in every arithmetic mode; no bias / BN / activation.
struct DeformConvParams {
  const float* in;      // [B,Ha,Wa,ldc], logical [B,H,W,C]
  const float* wt_off;  // deform_pack_offset_weights image
  const float* b_off;   // [18]
  const float* wt;      // deform_pack_weights image
  float* off;           // [B,Ho,Wo,18]: (row, column) offset of tap n = 3 ky + kx at channels (2 n, 2 n + 1)
  float* out;           // [B,Ho,Wo,C]
  unsigned* out_amax;   // range slot of out (|max| of what is stored) or nullptr
  int B, H, W, Ha, Wa, ldc, C, Ho, Wo;      // C in {128, 256, 512}; Ho = ceil(H / 2), Wo = ceil(W / 2)
};
size_t deform_offset_weight_elems(int C);
size_t deform_weight_elems(int C);
// HWIO [3][3][C][18] / [3][3][C][C] -> the kernels' images (host memory)
int deform_pack_offset_weights(const float* hwio, int C, float* dst);
int deform_pack_weights(const float* hwio, int C, float* dst);
// both kernels, in stream order (`between`: an event recorded after the offset kernel, for profiling)
int launch_deform_conv(const DeformConvParams& p, hipStream_t stream, hipEvent_t between = nullptr);

// ------------------------------------------------------- GroupNorm (group_norm.hip; --use_gn, reference nn.py:81-108)
// Per image and per group of C / 32 adjacent channels over the h x w view of x: mean and biased variance (f64 sums), then
// out = x * a + s with a = rsqrt(var + eps) * gamma[c], s = beta[c] - mean * a (f32, the reference's operand order), + the
// residual as res_mode says, optional ReLU.  x, out and res are NHWC f32 with pitches of their own.
constexpr int kGnGroups = 32;
struct GroupNormParams {
  const float* x;       // [B,Ha,Wa,ldc]; the view is rows [xoy, xoy + h), columns [xox, xox + w), channels < C of every image
  const float* gamma;   // [C]
  const float* beta;    // [C]
  const float* res;     // residual (see res_mode) or nullptr
  float* out;           // [B,oH,oW,out_ldc]; the view's pixels land at (oy, ox); nothing outside them is written.  May be x
  double* part;         // scratch [B][32][group_norm_parts][2]: per workgroup (sum, sum of squares)
  float* ab;            // scratch [B][2][C]: a, then s
  float* mean;          // [B][32]
  float* var;           // [B][32]
  unsigned* amax;       // range slot of out (|max| of what is stored) or nullptr
  int B, h, w, C;       // C % 32 == 0
  int Ha, Wa, ldc, xoy, xox;            // ldc, out_ldc, res_ldc multiples of 4
  int oH, oW, out_ldc, oy, ox;
  int res_mode;         // 0 none | 1 [B,res_H,res_W,res_ldc], same pixels | 2 nearest-2x upsample of [B,res_H,res_W,res_ldc]
  int res_H, res_W, res_ldc;
  int relu;
  float eps;
  int chunks;           // row ranges per image of the statistics pass; 0: group_norm_chunks (a function of h, w, C alone)
};
int group_norm_chunks(int h, int w, int C);
int group_norm_parts(int h, int w, int C, int chunks);      // partials per (image, group) that a launch with these sizes writes
int launch_group_norm(const GroupNormParams& p, hipStream_t stream);

// ------------------------------------------------------- GroupNorm of ROI tensors (group_norm_roi.hip; --use_gn + --use_conv_frcnn_head)
// The same arithmetic per ROI and group over the hw <= 64 pixels of x [R, hw, ldc], in one launch and one pass: no residual, no
// activation, no scratch.  32 <= C <= 512, C % 32 == 0; ldc, out_ldc multiples of 4; every pointer 16-byte aligned.
struct RoiGroupNormParams {
  const float* x;       // [R, hw, ldc]
  const float* gamma;   // [C]
  const float* beta;    // [C]
  float* out;           // [R, hw, out_ldc]; channels past C are not written.  May be x
  float* mean;          // [R][32] or nullptr
  float* var;           // [R][32] or nullptr
  unsigned* amax;       // range slot of out (|max| of what is stored) or nullptr
  int R, hw, C, ldc, out_ldc;
  float eps;
};
int launch_group_norm_roi(const RoiGroupNormParams& p, hipStream_t stream);

// ------------------------------------------------------- relation module of the box head (relation.hip; --add_relation_nn)
// The two kernels behind RM_r1 / RM_r2 (reference nn.py:115-190, 273-298) over the K proposal rows of each of B images on its
// own (blockIdx.z), of which the first n = min(count[b], K) are real.  16 heads; plain f32 in every arithmetic mode.
constexpr int kRelHeads = 16;        // `group` of relation_network
constexpr int kRelGeoDim = 64;       // geo_feat_dim
constexpr int kRelMaxK = 1024;       // proposals per image the attention kernel keeps a score row for
constexpr int kRelMaxD = 1024;       // widest feature vector (a multiple of 64)
constexpr int kRelGeoWeights = 4 * kRelGeoDim + kRelGeoDim + kRelGeoDim * kRelHeads + kRelHeads;      // 1360
inline int relation_kp(int K) { return (K + 3) & ~3; }      // row pitch of the bias tensor: 16-byte rows
// geometric bias: boxes [K,4] (x1, y1, x2, y2) -> bias [16, K, Kp], bias[h][i][j] = log(max(relu(a[i,j,h]), 1e-6)).  Entries with
// i >= n or j >= n are neither evaluated nor written
struct RelationGeoParams {
  const float* boxes;    // [B,K,4]
  const int* count;      // [B]: the images' proposal counts
  const float* wts;      // [1360]: geo_emb/W [4,64] | geo_emb/b [64] | geo_conv/W [64,16] | geo_conv/b [16]
  float* bias;           // [B, 16, K, Kp]
  int B, K, Kp;
};
int launch_relation_geo(const RelationGeoParams& p, hipStream_t stream);
// attention: S[i,h,j] = (Q_h[i] . K_h[j]) / sqrt(D / 16) + bias[h][i][j], P = softmax over j < n, O[i,h,:] = sum_j P[i,h,j] v[j,:].
// Rows i >= n of O are written as zeros; columns j >= n and rows >= n of q, k, v and bias are never read
struct RelationAttnParams {
  const float* q;        // [B K, D] at pitch qk_ldc; head h is columns h D/16 .. (h+1) D/16
  const float* k;        // [B K, D] at pitch qk_ldc
  const float* v;        // [B K, D] at pitch v_ldc: the module's input
  const float* bias;     // [B, 16, K, Kp]
  const int* count;      // [B]
  float* out;            // [B K, 16, D]
  unsigned* amax;        // range slot of out or nullptr
  int B, K, Kp, D, qk_ldc, v_ldc;
};
int launch_relation_attention(const RelationAttnParams& p, hipStream_t stream);

// ------------------------------------------------------- attention branch of the box head (att_head.hip; --use_att_frcnn_head)
// The two kernels around fastrcnn/att_trans (reference models.py:1064-1089); plain f32 in every arithmetic mode.  Every pointer
// 16-byte aligned.
// pool: x [R, 49, C] dense, C % 4 == 0 -> out [R, C], the 49 positions of a RoI added one after another in (h, w) order
struct AttPoolParams {
  const float* x;        // [R, 49, C]
  float* out;            // [R, C]
  unsigned* amax;        // range slot of out (|max| of what is stored) or nullptr
  int R, C;
};
int launch_att_pool(const AttPoolParams& p, hipStream_t stream);
// add: out [R, D] = h [R, D at row pitch ldh] + a [R, D]; D % 4 == 0, ldh % 4 == 0, ldh >= D
struct AttAddParams {
  const float* h;        // [R, D] at pitch ldh
  const float* a;        // [R, D]
  float* out;            // [R, D]
  unsigned* amax;        // range slot of out or nullptr
  int R, D, ldh;
};
int launch_att_add(const AttAddParams& p, hipStream_t stream);

// ------------------------------------------------------- EfficientDet tail (effdet_post.hip)
struct EffPostParams {
  const float* cls[5];     // per level [B, npix, ldc_cls]  (9 * ncls valid channels: anchor-major)
  const float* box[5];     // per level [B, npix, ldc_box]  (36 valid)
  int npix[5], anchor_off[6];   // anchors before level l; anchor_off[5] = total
  int ldc_cls, ldc_box, ncls, B;
  const float* anchors;    // [total, 4] y1,x1,y2,x2
  int k, max_out;
  float score_thresh, iou_thresh, image_scale;
  unsigned* keys;          // scratch [total * ncls]
  unsigned* hist;          // scratch [256]
  unsigned* state;         // scratch [5]
  unsigned long long* sel; // scratch [B, k]
  float* cand_boxes; float* cand_scores; int* cand_cls; int* cand_lvl;   // [B, k(,4)]
  float* out_boxes; float* out_scores; int* out_labels; int* out_levels; int* out_valid;   // [B, max_out(,4)], [B]
};
int launch_effdet_post(const EffPostParams& p, hipStream_t stream);

// ------------------------------------------------------- proposals (K6,K7,K8)
struct RpnLevel {
  const float* rpn;      // [B,h,w,kRpnCh]: ch 0..2 logits, 3+a*4+c deltas
  const float* anchors;  // [field,field,3,4]
  int h, w, field;
};
struct ProposalParams {
  RpnLevel lvl[5];
  int nlevels;
  int graph;             // ODT_GRAPH_SINGLE / MULTI semantics
  int B, K;
  int img_h, img_w;
  float nms_thresh, decode_clip;
  // workspace (device): per (b,level) sorted candidates and survivors
  float* cand_boxes;     // [B,L,K,4]
  float* cand_scores;    // [B,L,K]
  int* cand_count;       // [B,L]
  float* lvl_boxes;      // [B,L,K,4]
  float* lvl_scores;     // [B,L,K]
  int* lvl_count;        // [B,L]
  unsigned long long* chunk_keys;   // [B, total_chunks, K] per-chunk top-K keys (stage 1 of the select)
  // outputs
  float* props;          // [B,K,4]
  int* nprops;           // [B]
};
size_t proposal_workspace_bytes(int B, int L, int K);
int launch_proposals(const ProposalParams& p, hipStream_t stream);
int launch_topk(const float* scores, int n, int k, int* idx_out, hipStream_t stream);
int launch_nms(const float* boxes, const float* scores, int n, int max_out, float thresh,
               int* idx_out, int* n_out, hipStream_t stream);

// --------------------------------------------------------------- ROIAlign (K9,K14)
// A level one pixel high (wide) is defined, where the reference divides by h - 1 = 0: on that axis sample j lies at
// (y0 + sh / 2 - 0.5) + j * sh in level pixels (sh = box side / samples) and counts only where that is exactly 0 -- every
// sample off the single row (column) is the extrapolation value 0, as on any other level.
struct RoiAlignParams {
  const float* feat[5];  // NHWC [B,h,w,C] (sliced dims h,w ; pixel stride ldc); 5th level: EfficientDet P7
  int h[5], w[5], ldc[5], alloc_h[5], alloc_w[5];
  float inv_stride[5];
  const int* levels;     // optional [R_cap]: pyramid level of each box (value - level0 indexes feat[]); nullptr: FPN rule
  int level0;
  int C;
  const float* boxes;    // [R_cap,4] image coords
  const int* box_ind;    // [R_cap] or nullptr (then box r belongs to image r / per_image)
  int per_image;         // rows per image when box_ind == nullptr
  const int* count;      // device: number of valid rows per image [B] (nullptr: all R_cap)
  int R_cap;
  float* out_nhwc;       // [R_cap,7,7,C] or nullptr   (box-head input order h,w,c)
  float* out_nchw;       // [R_cap,C,7,7] or nullptr   (fpn_box_feat)
  float* pooled;         // [R_cap,C] or nullptr
  int out_size;          // 0 / 7: box head + features; 14: mask head (models.py:935-936)
  int pack_rows;         // with count: 1 = output rows packed over the valid rows of all images (final features, masks);
                         // 0 = row r stays row r, rows past count[b] untouched (box head: its consumers index b * per_image + j)
  unsigned* amax;        // optional range slot of out_nhwc (round 6: fc6 reads the RoI features on the fp16x2 kernels, which scale by the
                         // tensor's |max|).  With it the rows past count[b] are written as zeros instead of left stale: the recorded
                         // maximum must cover every row the consumer's GEMM reads
};
int launch_roi_align(const RoiAlignParams& p, hipStream_t stream);

// ------------------------------------------------------- mask head tail (models.py:951-962)
struct MaskSelectParams {
  const float* logits;   // [R_cap,14,14,4,ld]: deconv sub-pixel (dy,dx) major, class minor
  int ld;                // padded class stride
  const int* labels;     // [R_cap] 1-based foreground labels (device)
  const int* valid;      // [B] rows per image
  int B, per_image;
  float* masks;          // [R_cap,28,28]
};
int launch_mask_select(const MaskSelectParams& p, hipStream_t stream);

// ------------------------------------------------------- mask paste + COCO RLE (mask_rle.hip; obj_detect_tracking.py:715-739)
constexpr int kRleMaxH = 4096;         // frame rows (one LDS row-tap table per workgroup)
constexpr int kRleTransPerCol = 32;    // static bound: run boundaries per detection <= 32 * W0 + 1
struct MaskRleParams {
  const float* masks;    // [R,28,28] final_masks
  const float* boxes;    // [R,4] x1,y1,x2,y2 in network coordinates
  const int* valid;      // device count of detections (rows >= it produce nothing) or nullptr: n
  int R, n;
  int H0, W0;            // frame size
  float scale;           // boxes / scale = frame coordinates
  int cap;               // transitions per detection: kRleTransPerCol * W0 + 1
  int* trans;            // [R,cap] column-major run boundaries
  int* ntrans;           // [R] their number, -1 past the bound
  int* slen;             // [R] bytes of the compressed string
  char* str;             // the strings, packed in detection order
  unsigned* counts;      // the counts, packed (or nullptr)
};
int launch_mask_rle_runs(const MaskRleParams& p, hipStream_t stream);
int launch_mask_rle_strings(const MaskRleParams& p, hipStream_t stream);
// host result of one call (odt_rle_result points into it)
struct MaskRleHost {
  int n = 0, H0 = 0, W0 = 0;
  std::vector<char> str;
  std::vector<int64_t> off, coff;
  std::vector<int32_t> len;
  std::vector<uint32_t> counts;
};
// device buffer by name and size in bytes (a handle's persistent buffers, or the guarded buffers of odt_op_mask_rle)
typedef std::function<int(const char* name, size_t bytes, void** dev)> RleAlloc;
// runs kernel -> sizes to the host -> strings kernel -> strings (and counts) to the host, all on `st`
int run_mask_rle(MaskRleParams p, bool want_counts, hipStream_t st, const RleAlloc& alloc, MaskRleHost& out);

// ------------------------------------------------------- detection tail (K11,K12,K13)
struct DetectParams {
  int graph, B, K, C;          // C = num_class incl. BG
  const float* head_out;       // [B*K, ld] : cols [0,C) class logits, [C, C+4C) box logits
  int ld;
  const float* props;          // [B,K,4]
  const int* nprops;           // [B]
  int img_h, img_w;
  float reg_w[4];
  float decode_clip, score_thresh, nms_thresh;
  int per_im;
  // workspace
  float* dec_boxes;            // [B*K, C-1, 4]
  float* probs;                // [B*K, C]
  int* cls_keep;               // [B, C-1, per_im]
  int* cls_count;              // [B, C-1]
  // outputs (device)
  float* out_boxes;            // [B, per_im, 4]
  float* out_probs;            // [B, per_im]
  int* out_labels;             // [B, per_im]
  int* out_valid;              // [B]
};
int launch_detections(const DetectParams& p, hipStream_t stream);
int launch_class_nms(const DetectParams& p, hipStream_t stream);

// ----------------------------------------------------------------- tracker (K15)
// blocks: nn_cosine_blocks' table of <= 32-row gallery blocks (device copy); any_part: a track spans several blocks
bool nn_cosine_blocks(const int* seg, int T, std::vector<int>* blocks);
int launch_nn_cosine(const float* gallery, const int* seg, const int* blocks, int nblocks, bool any_part, int T, const float* dets, int N,
                     int D, double* cost, hipStream_t stream);
// host-to-host cosine nearest-neighbour call with persistent scratch and a stream of its own (tracker.hip)
struct CosineCtx {
  const Knobs knobs = knobs_read();   // the ODT_* overrides when the context was created (stream priority, timing)
  int device = -1;
  hipStream_t stream = nullptr;
  hipEvent_t done = nullptr;
  float* h_in = nullptr; float* d_in = nullptr; size_t cap_in = 0;        // packed [seg | gallery | detections]
  double* h_cost = nullptr; double* d_cost = nullptr; size_t cap_cost = 0;
  std::vector<int> blocks_scratch;                   // the call's block table (host)
  std::vector<void*> retired_host, retired_dev;      // outgrown buffers: released with the context (hipFree waits for the device)
  ~CosineCtx();
  // gal_rows[G] / det_rows[N]: pointers to the D-float rows (gathered into the pinned record); seg[T+1]; cost[T*N]
  int run(int dev, const float* const* gal_rows, int G, const int* seg, int T, const float* const* det_rows, int N,
          int D, double* cost);
};

}  // namespace odt
