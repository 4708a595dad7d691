// f32 implicit-GEMM convolution on the bf16 matrix pipe of gfx950 ("bf16x3 split"): weight images, the per-handle policy,
// and -- for every conv kernel, the exact-f32 one included -- the kernel table, the selection (conv_select), the validation
// of a record against its row (conv_check_variant) and the one launcher (launch_conv).  Kernels: conv_split3.hip (conv_split3_kernel /
// conv_split3k_kernel: 8 waves, LDS-DMA weight stages, three-stage ring; the default), conv_split1.hip (one-stage 4-wave
// loop: the 64-wide layers).  Same reference ops as conv_igemm.hip: nn.py:337-381 conv2d + :1771-1774 folded BN + ReLU,
// :503-521 residual, :949-1014 FPN lateral.  The arithmetic is described in conv_split_common.hpp.
// Scope: no residual, a same-shape residual or a nearest-2x upsampled one, an optional K-concatenated second A source
// (1x1), Cout % 64 == 0 (padded), Cin % 32 == 0, 16-byte-aligned output rows; everything else stays on the exact-f32 MFMA
// kernel (conv_select decides).
#include <array>

#include "conv_split_common.hpp"

namespace odt {

namespace {

// f32 weights [Cout][K] -> per-stage image of bf16 pieces (one thread per 8 consecutive k of a row)
// (kscale != nullptr: the row is multiplied by kscale[k] first -- a per-input-channel gate folded into a 1x1 conv's weights)
__global__ void split_weights_kernel(const float* __restrict__ wt, int Cout, int K, int SBN, int bk, unsigned short* __restrict__ img,
                                     const float* __restrict__ kscale) {
  const int nsl = K / bk, kgs = bk >> 3;     // stages along K, k-groups of 8 per stage
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;       // (n, k8), n over the padded Cout
  const long total = (long)cout_padded(Cout) * (K >> 3);
  if (idx >= total) return;
  const int n = (int)(idx / (K >> 3)), k8 = (int)(idx - (long)n * (K >> 3));
  const int tn = n / SBN, nn = n - tn * SBN, sl = k8 / kgs, kg = k8 - sl * kgs;
  for (int e = 0; e < 8; e += 2) {
    unsigned piece[3];
    float w0 = n < Cout ? wt[(size_t)n * K + k8 * 8 + e] : 0.f, w1 = n < Cout ? wt[(size_t)n * K + k8 * 8 + e + 1] : 0.f;
    if (kscale != nullptr) { w0 = w0 * kscale[k8 * 8 + e]; w1 = w1 * kscale[k8 * 8 + e + 1]; }
    split2(w0, w1, piece[0], piece[1], piece[2]);
    for (int q = 0; q < 3; ++q) {
      const size_t at = ((((size_t)(tn * nsl + sl) * 3 + q) * kgs + kg) * SBN + nn) * 8 + e;
      img[at] = (unsigned short)(piece[q] & 0xffffu);
      img[at + 1] = (unsigned short)(piece[q] >> 16);
    }
  }
}

// conv_split3_kernel's image: [n-tile][stage][piece][k-group 2][BN n][8 k], stage order = (16-channel slice, tap)
// for the first source, then the second source's slices; wt is [Cout][tap][Cin] (+ [Cin2] behind it)
__global__ void split_weights3_kernel(const float* __restrict__ wt, int Cout, int K, int SBN, int ntaps, int Cin,
                                      unsigned short* __restrict__ img, const float* __restrict__ kscale) {
  const int nst = K >> 4, nst1 = ntaps * (Cin >> 4);
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;       // (n, stage, k-group)
  const long total = (long)cout_padded(Cout) * nst * 2;       // n over the padded Cout: zero rows behind the last channel
  if (idx >= total) return;
  const int n = (int)(idx / (nst * 2)), rem = (int)(idx - (long)n * (nst * 2)), st = rem >> 1, kg = rem & 1;
  int k0;
  if (st < nst1) { const int cs = st / ntaps, tap = st - cs * ntaps; k0 = tap * Cin + cs * 16; }
  else k0 = ntaps * Cin + (st - nst1) * 16;
  k0 += kg * 8;
  const int tn = n / SBN, nn = n - tn * SBN;
  for (int e = 0; e < 8; e += 2) {
    unsigned piece[3];
    float w0 = n < Cout ? wt[(size_t)n * K + k0 + e] : 0.f, w1 = n < Cout ? wt[(size_t)n * K + k0 + e + 1] : 0.f;
    if (kscale != nullptr) { w0 = w0 * kscale[k0 + e]; w1 = w1 * kscale[k0 + e + 1]; }
    split2(w0, w1, piece[0], piece[1], piece[2]);
    for (int q = 0; q < 3; ++q) {
      const size_t at = ((((size_t)(tn * nst + st) * 3 + q) * 2 + kg) * SBN + nn) * 8 + e;
      img[at] = (unsigned short)(piece[q] & 0xffffu);
      img[at + 1] = (unsigned short)(piece[q] >> 16);
    }
  }
}

}  // namespace

size_t conv_split_weight_bytes(int Cout, int K) { return (size_t)cout_padded(Cout) * K * 6; }

// n-tile width of the configuration that takes a layer with this Cout (0: none)
int conv_split_bn(int Cout) { const int n = cout_padded(Cout); return n % 256 == 0 ? 256 : (n % 128 == 0 ? 128 : 64); }
int conv_split_bm(int Cout) { return cout_padded(Cout) % 256 == 0 ? 128 : 256; }

bool conv_split_supported(const ConvParams& p) {
  const double wbytes = (double)p.Cout * (p.kh * p.kw * p.Cin + (p.in2 != nullptr ? p.Cin2 : 0)) * 6.0;
  const bool res_ok = p.res_mode == 0 || (p.res_mode == 1 && p.res_H == p.Ho && p.res_W == p.Wo) ||
                      (p.res_mode == 2 && 2 * p.res_H >= p.Ho && 2 * p.res_W >= p.Wo);
  const bool src2_ok = p.in2 == nullptr || (p.kh == 1 && p.kw == 1 && p.Cin2 % 32 == 0 && p.in2_ldc % 4 == 0);
  // a channel count that is not a multiple of 64 needs room for the padded n-tile in the output (and residual) rows
  const int np = cout_padded(p.Cout);
  const bool pad_ok = np == p.Cout || (p.Cout >= 16 && p.out_ldc >= np && (p.res_mode == 0 || p.res_ldc >= np));
  return pad_ok && p.Cin % 32 == 0 && src2_ok && res_ok && p.out_ldc % 4 == 0 &&
         p.in_ldc % 4 == 0 && wbytes < 2147483648.0;
}

// ---- policy: which convs take the split kernels, and which family.  A model's policy is fixed when its handle is
// created (odt_config.conv_arith / conv_split_family -> odt_create) and recorded with the handle (odt_describe); the
// ODT_CONV_* overrides (debug / A-B) of the handle's knob snapshot go on top of it (conv_policy_with_knobs) -- or those of
// the call for the stand-alone test entry points (odt_op_conv2d ...), which have no handle.
ConvPolicy conv_policy_default() {
  ConvPolicy q;
  q.arith = 1;            // bf16x3 split where it pays (same-box A/B at b=8 1080p: 116 -> 178 FPS, parity suite green)
  q.family = 2;           // fp16x2 kernels where a layer has 256-row tiles and a recorded input range (same-box A/B at b=8
                          // 1080p: 188 -> 259 FPS, profiles/r03_fp16x2_vs_bf16x3_ab.txt), conv_split3_kernel where its tiles fill the chip
  q.min_tiles = 256;      // one- / two-stage kernels: A/B at b=8 and b=1: 256 > 384 > 128 >> 64
  q.min_tiles3 = 200;
  q.min_k = 64;           // A/B at b=8: K >= 256: 155.0, >= 128: 156.2, >= 64: 156.6 FPS
  q.h2s_maxk = 0;         // fp16x2: reductions up to this K take the 128 x 128 two-per-CU tile (A/B knob; measured: no gain)
  q.h2_few_tiles = true;  // fp16x2: layers without enough 256-row tiles take 128 x 128 tiles instead of bf16x3 + split-K
  q.h2_n64 = true;        // fp16x2: the 64-wide layers too
  q.h2k_fewrows = 1;  // fp16x2 kw-reuse kernel on 256 x 128 tiles without split-K where those fill the chip (round-6 A/B knob)
  q.h2k_splitk = true;    // fp16x2 kw-reuse kernel with split-K for the stride-1 KH x 3 layers of few rows (ODT_CONV_H2K_SPLITK=0: A/B)
  q.fill_div = 6;         // split-K layers are taken when tiles x ranges reach min_tiles3 / fill_div workgroups (b = 1: fc6 / fc7 leave the
                          // exact-f32 kernel: 139.4 -> 144.9 FPS same box, profiles/r04_b1_filldiv_ab.txt; ODT_CONV_SPLIT3_FILLDIV: A/B)
  q.h2_bm64 = 3;          // fp16x2: 64 x 128 two-wave tiles instead of 128 x 128 + split-K where only those fill the chip: 0 off | 1 for
                          // reductions up to K = 1024 (no split-K at all) | 2 also the longer ones, cut in two | 3 = 1 on 64 x 64 tiles (ODT_CONV_H2_BM64: A/B)
  q.h2_n64_bm512 = 1;     // fp16x2 kw-reuse kernel on 64-wide layers: 512 x 64 tiles (eight waves stacked along M: 24 MFMAs per wave and
                          // stage instead of 12) where they fill the chip (res2 conv2 1.035 -> 0.897 ms, same box); 0 off, 2 wherever
                          // the shape allows, the generic kernel included (tests)
  q.min_bn = 0; q.force_bm3 = 0; q.splitk_max = 8; q.force_splitk = 0; q.kw_reuse = true; q.kwr_n64 = true; q.src2 = true; q.res2 = true;
  return q;
}

ConvPolicy conv_policy_with_knobs(ConvPolicy q, const Knobs& kn) {
  auto geti = [&](Knob k, long* dst) {
    const KnobVal& e = kn.get(k);
    if (e.set) *dst = e.i;
  };
  long v;
  v = q.arith; geti(K_CONV_SPLIT, &v); q.arith = v != 0 ? 1 : 0;
  v = q.family; geti(K_CONV_SPLIT_PIPE, &v); q.family = v >= 3 ? 3 : (v == 2 ? 2 : 1);
  geti(K_CONV_SPLIT_MINTILES, &q.min_tiles);
  geti(K_CONV_SPLIT3_MINTILES, &q.min_tiles3);
  v = q.min_k; geti(K_CONV_SPLIT_MINK, &v); q.min_k = (int)v;
  v = q.min_bn; geti(K_CONV_SPLIT_MINBN, &v); q.min_bn = (int)v;
  v = q.h2s_maxk; geti(K_CONV_H2S_MAXK, &v); q.h2s_maxk = (int)v;
  v = q.h2_few_tiles; geti(K_CONV_H2_FEW_TILES, &v); q.h2_few_tiles = v != 0;
  v = q.h2_n64; geti(K_CONV_H2_N64, &v); q.h2_n64 = v != 0;
  v = q.h2_n64_bm512; geti(K_CONV_H2_N64_BM512, &v); q.h2_n64_bm512 = (int)v;
  v = q.h2_bm64; geti(K_CONV_H2_BM64, &v); q.h2_bm64 = (int)v;
  v = q.h2k_splitk; geti(K_CONV_H2K_SPLITK, &v); q.h2k_splitk = v != 0;
  v = q.h2k_fewrows; geti(K_CONV_H2K_FEWROWS, &v); q.h2k_fewrows = (int)v;
  v = q.fill_div; geti(K_CONV_SPLIT3_FILLDIV, &v); q.fill_div = v < 1 ? 1 : (int)v;
  v = q.force_bm3; geti(K_CONV_SPLIT3_BM, &v); q.force_bm3 = (int)v;
  v = q.splitk_max; geti(K_CONV_SPLIT3_SPLITK, &v); q.splitk_max = v < 1 ? 1 : (v > 16 ? 16 : (int)v);
  v = q.kw_reuse; geti(K_CONV_SPLIT3_KWR, &v); q.kw_reuse = v != 0;
  v = q.kwr_n64; geti(K_CONV_SPLIT3_KWR_N64, &v); q.kwr_n64 = v != 0;
  v = q.force_splitk; geti(K_CONV_SPLIT3_FORCE_SPLITK, &v); q.force_splitk = v < 0 ? 0 : (v > 16 ? 16 : (int)v);
  v = q.src2; geti(K_CONV_SPLIT_SRC2, &v); q.src2 = v != 0;      // 0 keeps the fused stage-entry convs on the f32 kernel
  v = q.res2; geti(K_CONV_SPLIT_RES2, &v); q.res2 = v != 0;      // 0 keeps the FPN laterals on the f32 kernel
  return q;
}

// ---- the kernel table --------------------------------------------------------------------------------------------------
// Rows come from the family files (the kernels live in their anonymous namespaces); built once, on first use.
static const ConvKernelRow* conv_table() {
  static const std::array<ConvKernelRow, CV_COUNT> table = [] {
    std::array<ConvKernelRow, CV_COUNT> t{};
    conv_rows_f32(t.data()); conv_rows_split1(t.data()); conv_rows_split3(t.data()); conv_rows_h2(t.data());
    conv_rows_h2d(t.data()); conv_rows_h2k(t.data()); conv_rows_stem(t.data());
    return t;
  }();
  return table.data();
}

const ConvKernelRow& conv_variant_row(int variant) { return conv_table()[variant > 0 && variant < CV_COUNT ? variant : CV_NONE]; }

int conv_variant_find(int family, int bm, int bn, unsigned flags) {
  for (int v = 1; v < CV_COUNT; ++v) {
    const ConvKernelRow& r = conv_table()[v];
    if (r.family == family && r.bm == bm && r.bn == bn && r.flags == flags && r.launch != nullptr) return v;
  }
  return CV_NONE;
}

int conv_variant_fused_tail(int variant) {
  const ConvKernelRow& r = conv_variant_row(variant);
  if (r.family != CF_H2 || r.flags != CVF_KWR) return CV_NONE;
  return conv_variant_find(CF_H2, 256, r.bn, CVF_KWR | CVF_FTAIL);
}

void conv_use_variant(ConvParams& p, int variant, int splitk, int reduce_blocks) {
  p.variant = variant; p.splitk = splitk; p.reduce_blocks = reduce_blocks;
}

// ---- shape predicates (selection and validation share them) ------------------------------------------------------------
int conv_k(const ConvParams& p) { return p.kh * p.kw * p.Cin + (p.in2 != nullptr ? p.Cin2 : 0); }
static long conv_tiles(const ConvParams& p, int bm, int bn) { return (((long)p.B * p.Ho * p.Wo + bm - 1) / bm) * (cout_padded(p.Cout) / bn); }

// stride-1 KH x 3 convs over rows of the output's pitch: the kw taps share a staged run of pixels
bool conv_kwr_fits(const ConvParams& p) {
  return p.kw == 3 && p.stride == 1 && p.in_Wa == p.Wo && p.in2 == nullptr && 2 * p.dil <= 4 && p.kh * 3 <= 30;
}
// ... and images large enough for it to pay
static bool conv_kwr_pays(const ConvParams& p) { return conv_kwr_fits(p) && p.Ho * p.Wo >= 256; }

// fp16x2 pieces: source tensor(s) that come with a recorded |max|, 32-channel slices
bool conv_h2_sources_ok(const ConvParams& p) {
  return p.in_amax != nullptr && (p.in2 == nullptr || (p.in2_amax != nullptr && p.Cin2 % 32 == 0)) && p.Cin % 32 == 0 && p.nlvl <= 1 &&
         p.kh * p.kw <= 32;
}

// layers of few rows: the split-K factor that brings `tiles` workgroups to `target`, at most `cap`, at least `min_stages` of
// the reduction's `stages` per range
static int splitk_for(long target, long tiles, int cap, int stages, int min_stages) {
  int k = (int)((target + tiles - 1) / tiles);
  if (k > cap) k = cap;
  while (k > 1 && stages / k < min_stages) --k;
  return k;
}

// ---- selection -----------------------------------------------------------------------------------------------------------
namespace {

struct Tile { int family, bm, bn; unsigned flags; int splitk; };

// what every rule sees: the conv, the policy, and conv_split3_kernel's way of filling the chip with this layer if it has one
// (fit: 256-row tiles, 128-row tiles, or 128-row tiles with the reduction cut into split-K ranges -- layers of few output
// rows: everything at b=1 below res3, the box head's FC layers, the coarse pyramid levels)
struct Sel {
  const ConvParams& p; const ConvPolicy& q;
  long M; int K, np, bn0;
  bool fit; int b3, n3, k3;
  bool kwr3;       // the fit runs on the kw-reuse kernel
  bool h2;         // the fp16x2 kernels may take the fit's layer
};

int forced_splitk(const Sel& s, int stages) {
  return s.q.force_splitk > 1 && s.p.in2 == nullptr && stages >= s.q.force_splitk ? s.q.force_splitk : 1;
}

void split3_fit(Sel& s) {
  const ConvParams& p = s.p; const ConvPolicy& q = s.q;
  s.fit = false; s.b3 = 0; s.n3 = s.bn0; s.k3 = 1;
  if (q.family < 2 || s.bn0 == 0 || p.kh * p.kw > 32 || s.K < 32 || p.Cin % 16 != 0) return;
  const int nsteps = s.K >> 4;
  if (q.force_bm3 == 256 || (q.force_bm3 == 128 && s.bn0 >= 128)) { s.fit = true; s.b3 = q.force_bm3; s.k3 = forced_splitk(s, nsteps); return; }
  // (64-wide layers stay on the one-stage 256 x 64 tile: a 64 x 32 wave tile reads too many fragments per MFMA --
  // same-box A/B at b=8: res2 conv2 132 vs 118 TF, conv0 136 vs 112)
  // ... except where the kw-reuse kernel applies: with a third of the A-side work the 64-wide 3x3 layers (res2 conv2)
  // come out ahead on it (same-box A/B in profiles/r02_kw_reuse_n64_ab.txt)
  if (s.bn0 < 128 && !(q.kw_reuse && q.kwr_n64 && conv_kwr_pays(p))) return;
  const long t256 = conv_tiles(p, 256, s.bn0), t128 = conv_tiles(p, 128, s.bn0);
  if (t256 >= q.min_tiles3) { s.fit = true; s.b3 = 256; s.k3 = forced_splitk(s, nsteps); return; }
  if (s.bn0 < 128) return;
  if (t128 >= q.min_tiles3) { s.fit = true; s.b3 = 128; s.k3 = forced_splitk(s, nsteps); return; }
  if (q.splitk_max > 1 && p.in2 == nullptr) {
    const int k = splitk_for(q.min_tiles3, t128, q.splitk_max, nsteps, 8);            // at least eight stages per range
    if (k > 1 && t128 * k >= q.min_tiles3 / q.fill_div) { s.fit = true; s.b3 = 128; s.k3 = k; }
  }
}

// The rules, tried in order; the first that applies decides.  A rule returns false to pass.
typedef bool (*Rule)(const Sel& s, Tile& t);
#define TILE(fam, bm, bn, flags, sk) (t = Tile{fam, bm, bn, flags, sk}, true)

// not a layer for the split kernels at all (conv_split_supported: scope; policy switches; reductions too short to pay)
bool rule_exact_f32_outside_policy(const Sel& s, Tile& t) {
  const ConvParams& p = s.p; const ConvPolicy& q = s.q;
  if (q.arith != 0 && conv_split_supported(p) && s.K >= q.min_k && (p.in2 == nullptr || q.src2) && (p.res_mode != 2 || q.res2) &&
      s.bn0 >= q.min_bn) return false;
  return TILE(CF_F32, 0, 0, 0, 0);
}
// one- / two-stage kernels: below one workgroup per CU the exact-f32 kernel's smaller tiles fill the chip better
bool rule_exact_f32_too_few_tiles(const Sel& s, Tile& t) {
  if (s.fit || conv_tiles(s.p, conv_split_bm(s.p.Cout), s.bn0) >= s.q.min_tiles) return false;
  return TILE(CF_F32, 0, 0, 0, 0);
}
// fp16x2, a 64-wide layer whose fit is NOT the kw-reuse kernel (a forced tile height took it past the size rule of
// rule_h2_n64_small_tiles): same choice as there
bool rule_h2_n64_forced(const Sel& s, Tile& t) {
  if (!s.h2 || s.n3 != 64 || s.kwr3 || s.p.in2 != nullptr) return false;
  return TILE(CF_H2, cout_padded(s.p.Cout) == 64 && s.q.h2_n64_bm512 == 2 ? 512 : 128, 64, 0, 1);      // (512: tests only, see below)
}
// fp16x2 on the fit's 256-row tiles (n-tile at least 128 wide, or the kw-reuse kernel)
bool rule_h2_256_rows(const Sel& s, Tile& t) {
  const ConvParams& p = s.p; const ConvPolicy& q = s.q;
  if (!s.h2 || s.b3 != 256 || (s.n3 == 64 && !s.kwr3) || (s.K >> 5) < s.k3) return false;
  TILE(CF_H2, 256, s.n3, s.kwr3 ? CVF_KWR : 0u, s.k3);
  // 64-wide kw-reuse layers (res2 conv2): 512 x 64 tiles, a 64 x 64 wave tile (a tile may cross ONE image boundary)
  if (s.n3 == 64 && s.kwr3 && s.k3 == 1 && p.Ho * p.Wo >= 512 && s.np == 64 &&
      (q.h2_n64_bm512 == 2 || (q.h2_n64_bm512 == 1 && (s.M + 511) / 512 >= q.min_tiles3)))
    t.bm = 512;
  // (A/B knob, off: short reductions on 128 x 128 tiles, two workgroups per CU in different phases -- measured no gain:
  // res4 conv3 4.28 -> 4.38 ms, res2 / res3 conv3 and the laterals 3-12 % slower, profiles/r03_h2_small_tile_ab.txt)
  if (!s.kwr3 && s.k3 == 1 && s.K <= q.h2s_maxk && conv_tiles(p, 128, 128) >= q.min_tiles3) { t.bm = 128; t.bn = 128; }
  return true;
}
// stride-1 KH x 3 layers of few rows (res3 / res4 conv2 at b = 1, the P5 3x3s at b = 8): the kw-reuse kernel on
// 256 x 128 tiles with the (slice, kh) groups cut into ranges -- a third of the activation-side work of the
// generic kernel's 128 x 128 split-K tiles (same-box A/B at b = 1, profiles/r04_b1_h2k_splitk_ab.txt: res4 conv2
// 83 -> 78 us per layer; the 128-wide res3 conv2 lost, 65 -> 74 us, and keeps the generic kernel)
// (round 6: the 256 x 128 kw-reuse tiles WITHOUT split-K where they alone fill the chip -- res5 conv2 at b = 8:
// 64 x 4 = 256 tiles, one round, a third of the generic kernel's activation-side work -- instead of its 128 x 128
// tiles: 0.503 -> 0.376 ms for the two layers, 320.3 -> 321.8 FPS same box, profiles/r06_res5_conv2_kwr_tiles_ab.txt;
// ODT_CONV_H2K_FEWROWS=0: A/B)
bool rule_h2k_few_rows(const Sel& s, Tile& t) {
  const ConvParams& p = s.p; const ConvPolicy& q = s.q;
  if (!s.h2 || s.b3 != 128 || s.n3 < 256 || !q.h2k_splitk || !q.kw_reuse || !conv_kwr_pays(p) || q.splitk_max <= 1 || q.force_splitk > 1) return false;
  const long t256 = conv_tiles(p, 256, 128);
  const int k = splitk_for(q.min_tiles3, t256, q.splitk_max, p.kh * (p.Cin >> 5), 3);
  if (k <= 1 ? !(q.h2k_fewrows && t256 >= q.min_tiles3) : t256 * k < q.min_tiles3 / 2) return false;
  return TILE(CF_H2, 256, 128, CVF_KWR, k <= 1 ? 1 : k);
}
// (A/B, ODT_CONV_H2K_FEWROWS=2: the same for the dense 1x1 layers of few rows -- res5 conv1 -- on conv_h2_kernel<2, 4>)
bool rule_h2_dense_few_rows(const Sel& s, Tile& t) {
  const ConvParams& p = s.p; const ConvPolicy& q = s.q;
  if (!s.h2 || s.b3 != 128 || s.n3 < 256 || q.h2k_fewrows < 2 || p.kh * p.kw != 1 || p.in2 != nullptr || conv_tiles(p, 256, 128) < q.min_tiles3) return false;
  return TILE(CF_H2, 256, 128, 0, 1);
}
// too few 256-row tiles (res5, P5 at b=8; everything below res3 at b=1), first choice: 64 x 128 tiles (two waves, three
// workgroups per CU) fill the chip without cutting the reduction: no partial slabs, no combine pass (b = 1: res4 has
// 128 x 2 ... 8 such tiles)
// (same-box A/B at b = 1, profiles/r04_b1_bm64_ab.txt: res4 conv1, K = 1024: 62.8 -> 44.4 us per layer; the K = 2304
// 3x3 layers lose without split-K -- 72 serial stages: 81.7 -> 105.8 us -- and take the tiles with the reduction cut in two)
bool rule_h2_64_rows(const Sel& s, Tile& t) {
  const ConvParams& p = s.p; const ConvPolicy& q = s.q;
  if (!s.h2 || s.b3 != 128 || s.n3 < 128 || !q.h2_few_tiles) return false;
  if (!(q.h2_bm64 > 0 && conv_tiles(p, 128, 128) < q.min_tiles3 && conv_tiles(p, 64, 128) >= q.min_tiles3 && q.force_splitk <= 1 &&
        (s.K <= 1024 || (q.h2_bm64 == 2 && p.in2 == nullptr)))) return false;
  // 64 x 64 tiles (conv_h2_kernel<1, 1>: twice the workgroups once more) for the reductions that stay whole: same box, b = 1,
  // res4 conv1 44.0 -> 41.7 us per layer, 171.6 -> 174.3 FPS (profiles/r04_b1_tiles64_ab.txt; taking 64 x 128 tiles also
  // where 128 x 128 ones give fewer than four workgroups per CU -- res4 conv3 -- lost: 33 -> 46 us per layer)
  return TILE(CF_H2, 64, q.h2_bm64 == 3 && s.K <= 1024 ? 64 : 128, 0, s.K <= 1024 ? 1 : 2);
}
// ... second choice: 128 x 128 tiles on 4 waves -- without split-K where they fill the chip (res5 conv2 0.690 -> 0.465 ms,
// conv1 0.338 -> 0.219, same file), else with the reduction cut into ranges (at least four 32-channel stages each)
// (two of these workgroups share a CU: the chip has twice min_tiles3 slots for them -- res4 at b=1 ran its 128 tiles
// x 2 ranges one 4-wave workgroup per CU, a single wave per SIMD)
bool rule_h2_128_rows(const Sel& s, Tile& t) {
  const ConvParams& p = s.p; const ConvPolicy& q = s.q;
  if (!s.h2 || s.b3 != 128 || s.n3 < 128 || !q.h2_few_tiles) return false;
  const long t128 = conv_tiles(p, 128, 128);
  int k = 1;
  if (t128 < q.min_tiles3 && q.splitk_max > 1 && p.in2 == nullptr) k = splitk_for(2 * q.min_tiles3, t128, q.splitk_max, s.K >> 5, 4);
  if (forced_splitk(s, s.K >> 5) > 1) k = q.force_splitk;
  if (t128 * k < q.min_tiles3 / 2) return false;
  return TILE(CF_H2, 128, 128, 0, k);
}
// conv_split3_kernel / conv_split3k_kernel on the fit
bool rule_split3(const Sel& s, Tile& t) {
  if (!s.fit) return false;
  return TILE(CF_SPLIT3, s.b3, s.n3, s.kwr3 ? CVF_KWR : 0u, s.k3);
}
// the 64-wide layers outside the kw-reuse kernel (conv0, res2 conv1): fp16x2 pieces on 128 x 64 tiles of 4 waves (three
// workgroups per CU) instead of the one-stage bf16x3 loop
// 512 x 64 tiles on 8 waves stacked along M for these layers (conv0, res2 conv1): built, tested, and NOT the default --
// same-box A/B at b=8 1080p: conv0 0.767 -> 0.888 ms, res2 conv1 0.555 -> 0.587 (three 4-wave workgroups per CU in different
// phases hide these HBM-bound layers' loads and stores better than one 8-wave workgroup; profiles/r04_n64_bm512_ab.txt)
bool rule_h2_n64_small_tiles(const Sel& s, Tile& t) {
  const ConvParams& p = s.p; const ConvPolicy& q = s.q;
  if (q.family != 2 || !q.h2_n64 || s.bn0 != 64 || !conv_h2_sources_ok(p) || p.lvl_scale != nullptr || p.head_wt != nullptr || p.in2 != nullptr ||
      conv_tiles(p, 128, 64) < q.min_tiles) return false;
  return TILE(CF_H2, s.np == 64 && q.h2_n64_bm512 == 2 ? 512 : 128, 64, 0, 1);
}
// the one-stage BK = 32 kernel (family 1: everywhere; otherwise the 64-wide layers the rules above left)
bool rule_split1(const Sel& s, Tile& t) { return TILE(CF_SPLIT1, conv_split_bm(s.p.Cout), s.bn0, 0, 1); }
#undef TILE

const Rule kRules[] = {rule_exact_f32_outside_policy, rule_exact_f32_too_few_tiles, rule_h2_n64_forced,     rule_h2_256_rows,
                       rule_h2k_few_rows,             rule_h2_dense_few_rows,       rule_h2_64_rows,        rule_h2_128_rows,
                       rule_split3,                   rule_h2_n64_small_tiles,      rule_split1};

// the exact-f32 kernel's tile / stages / loop style
int select_exact_f32(const ConvParams& p, const Knobs& k) {
  const long M = (long)p.B * p.Ho * p.Wo;
  const long tiles128 = ((M + 127) / 128) * ((p.Cout + 127) / 128);
  int tile = (int)k.get_long(K_CONV_TILE, 0);   // 0 auto | 1: 128x64 | 2: 64x64 | 3: 128x128  (ODT_CONV_TILE: tuning / test knob)
  // short reductions (K <= 384: EfficientNet / BiFPN 1x1 convs, the res2 / res3 1x1 layers): the
  // 64x64 tile wins -- more workgroups per CU hide the per-tile prologue / epilogue that a two-to-
  // twelve-slice main loop cannot amortise (measured per layer; ODT_CONV_SMALLK=0 for the A/B)
  const bool smallk = !k.off(K_CONV_SMALLK);
  const int Kfull = conv_k(p);
  if (tile == 0) tile = p.Cout <= 64 ? 1 : ((tiles128 < 384 || (smallk && Kfull <= 384)) ? 2 : 3);
  // LDS stages: the single-stage / 3-workgroups-per-CU variant wins everywhere (measured per
  // layer, profiles/) except the long 1x1 reductions on the 128x128 tile (res4 conv1, K = 1024:
  // every slice is fresh HBM data, the two-slice register+LDS prefetch of ST = 2 hides it better).
  int stages = (tile == 3 && p.kh * p.kw == 1 && p.Cin >= 1024) ? 2 : 1;
  if (k.get(K_CONV_STAGES).i == 1 || k.get(K_CONV_STAGES).i == 2) stages = (int)k.get(K_CONV_STAGES).i;     // tuning knob: force 1 or 2
  // Loop style (measured per layer, profiles/r01_conv_fine_vs_coarse*.txt): the fine-grained
  // interleave keeps the matrix pipe of a CU busy when few workgroups share it (single-round
  // launches: everything at b=1) and on long reductions; on short reductions with several rounds
  // the workgroups in prologue / epilogue need the issue slots that a never-stalling main loop
  // takes, and the coarse loop wins.
  const int BMt = tile == 2 ? 64 : 128, BNt = tile == 3 ? 128 : 64;
  const long tiles = ((M + BMt - 1) / BMt) * ((p.Cout + BNt - 1) / BNt);
  const long slots = 256L * (stages == 2 ? 2 : (tile == 3 ? 3 : 4));
  bool fine = stages == 2 || (tile != 2 && (tiles <= slots || tile == 1 || (Kfull >= 1024 && tiles >= 2 * slots)));
  if (tile == 2) fine = tiles >= 384 && tiles <= slots;
  if (k.get(K_CONV_FINE).c0 == '0' || k.get(K_CONV_FINE).c0 == '1') fine = k.get(K_CONV_FINE).c0 == '1';       // tuning knob: force 0 or 1
  return conv_variant_find(CF_F32, BMt, BNt, (stages == 2 ? CVF_ST2 : 0u) | (fine ? CVF_FINE : 0u));
}

}  // namespace

ConvChoice conv_select(const ConvParams& p, const ConvPolicy& q, const Knobs& k) {
  Sel s{p, q, (long)p.B * p.Ho * p.Wo, conv_k(p), cout_padded(p.Cout), conv_split_bn(p.Cout), false, 0, 0, 1, false, false};
  split3_fit(s);
  s.kwr3 = s.fit && q.kw_reuse && s.b3 == 256 && s.k3 == 1 && (s.n3 >= 128 || q.kwr_n64) && conv_kwr_pays(p);
  // fp16x2 pieces: tiles at least 128 wide (or the 64-wide layers too) whose source tensor(s) come with a recorded |max|
  s.h2 = s.fit && q.family == 2 && (s.n3 >= 128 || q.h2_n64) && conv_h2_sources_ok(p) && p.lvl_scale == nullptr && p.head_wt == nullptr;
  Tile t{CF_F32, 0, 0, 0, 0};
  for (const Rule rule : kRules)
    if (rule(s, t)) break;
  if (t.family == CF_F32) return ConvChoice{select_exact_f32(p, k), 0, 0};
  // the dense 1x1 reductions on two-wave fp16x2 tiles: double stages (conv_h2d.hip; ODT_CONV_H2_BK64=0: the single-stage kernel, A/B)
  if (t.family == CF_H2 && t.bm == 64 && t.splitk == 1 && conv_h2d_fits(p) && !k.off(K_CONV_H2_BK64)) t.flags |= CVF_DSTAGE;
  // split-K combine pass: at most two blocks per CU (same-box A/B at b = 1: 2048 blocks 150.4, 512 167.5, 256 166.8, 128 159.6
  // FPS): every block ends with a conditional atomicMax on the ONE range slot of the output, and the blocks of a short pass all
  // find the slot empty -- 2040 same-address atomics serialised in L2 made this pass 35 us per call at b = 1 (1.2 ms of the
  // 6.8 ms frame, profiles/r04_kernel_stats_bench_b1_single_before.txt)
  const long capv = k.get_long(K_SPLIT_REDUCE_BLOCKS, 512L);
  return ConvChoice{conv_variant_find(t.family, t.bm, t.bn, t.flags), t.splitk, capv > 0 ? (int)capv : 512};
}

int conv_finish(ConvParams& p, const Knobs& k) {
  conv_prepare(p);
  if (k.get(K_CONV_DEBUG).i != 0) p.debug = (int)k.get(K_CONV_DEBUG).i;
  if (p.wt_split == nullptr) conv_use_variant(p, select_exact_f32(p, k), 0);
  return conv_check(p);
}

// ---- validation: the record against its row ------------------------------------------------------------------------------
int conv_check_variant(const ConvParams& p) {
  const ConvKernelRow& r = conv_variant_row(p.variant);
  const bool split3 = p.wt_split != nullptr && r.family == CF_SPLIT3;
  ODT_CHECK(p.nlvl <= 1 || (split3 && p.splitk <= 1 && p.nlvl <= 5 && p.head_wt == nullptr),
            "conv: per-row-range epilogue constants need a conv_split3 kernel without split-K");
  if (p.wt_split == nullptr) {
    ODT_CHECK(p.variant == CV_NONE || r.family == CF_F32, "conv: a split-kernel row without a weight image");
    return 0;
  }
  ODT_CHECK(r.launch != nullptr && r.family != CF_F32, "conv: the record's variant names no split-kernel row of the table");
  ODT_CHECK(cout_padded(p.Cout) % r.bn == 0, "conv: the row's n-tile does not divide the padded channel count");
  const long M = (long)p.B * p.Ho * p.Wo;
  const int sk = p.splitk > 1 ? p.splitk : 1;
  const bool kwr = (r.flags & CVF_KWR) != 0;
  ODT_CHECK(sk == 1 || p.reduce_blocks > 0, "conv: split-K without a combine-pass grid");
  if (r.flags & CVF_STEM) {
    ODT_CHECK(conv_stem_fits(p) && p.out != nullptr && p.out_H == (p.Ho + 1 - 3) / 2 + 1 && p.out_W == (p.Wo + 1 - 3) / 2 + 1 &&
              p.out_oy == 0 && p.out_ox == 0, "conv stem: unsupported shape");
  } else if (r.family == CF_H2) {
    ODT_CHECK((r.bm != 512 || !kwr || p.Ho * p.Wo >= 512) && conv_h2_sources_ok(p) && p.h2_chinv != nullptr &&
              (!(r.flags & CVF_DSTAGE) || (sk == 1 && conv_h2d_fits(p))),
              "conv h2: unsupported tile / shape, or no recorded input range");
    ODT_CHECK(sk == 1 || (p.partial != nullptr && p.in2 == nullptr && p.head_wt == nullptr && (p.kh * p.kw * p.Cin >> 5) >= sk),
              "conv h2: split-K needs a partial buffer, a single source and at least one stage per range");
    ODT_CHECK((p.f_wt != nullptr) == ((r.flags & CVF_FTAIL) != 0), "conv h2: a fused 1x1 tail needs the kw-reuse kernel");
    if (kwr) {
      ODT_CHECK(conv_kwr_fits(p) && (sk == 1 || (r.bm == 256 && r.bn >= 128 && p.f_wt == nullptr && p.kh * (p.Cin >> 5) >= sk)), "conv h2k: unsupported shape");
      ODT_CHECK(p.f_wt == nullptr || (r.bn == p.Cout && p.head_wt == nullptr && p.res_mode == 0 && p.relu <= 1 && p.f_cout % 32 == 0 &&
                                      p.f_cout > 0 && p.f_cout <= 1024 && p.f_out != nullptr && p.f_chinv != nullptr && p.f_bias != nullptr && p.f_out_ldc % 4 == 0 &&
                                      (p.f_res == nullptr || p.f_res_ldc % 4 == 0) && (double)M * p.f_out_ldc * 4.0 < 2147483648.0 &&
                                      (p.f_res == nullptr || (double)M * p.f_res_ldc * 4.0 < 2147483648.0)),
                "conv h2k: unsupported fused 1x1 tail");
    }
  } else if (r.family == CF_SPLIT3) {
    ODT_CHECK(p.Cin % 16 == 0 && p.kh * p.kw <= 32, "conv split3: unsupported tile / shape");
    ODT_CHECK(sk == 1 || (p.partial != nullptr && p.in2 == nullptr && (p.kh * p.kw * p.Cin >> 4) >= sk),
              "conv split3: split-K needs a partial buffer, a single source and at least one stage per range");
    ODT_CHECK(!kwr || (sk == 1 && conv_kwr_fits(p)), "conv split3k: unsupported shape");
  } else {
    ODT_CHECK(sk == 1 && r.bm == conv_split_bm(p.Cout) && r.bn == conv_split_bn(p.Cout), "conv split1: the tile follows from the channel count");
  }
  return 0;
}

// ---- the launcher ----------------------------------------------------------------------------------------------------------
int launch_conv(const ConvParams& p, const ConvParams* dev, hipStream_t stream) {
  const ConvKernelRow& r = conv_variant_row(p.variant);
  ODT_CHECK(r.launch != nullptr, "conv: launch of a record without a kernel variant");
  const int sk = p.splitk > 1 ? p.splitk : 1;
  unsigned grid;
  if (r.flags & CVF_STEM) {      // persistent workgroups: the one grid that is not tiles x ranges
    if (conv_stem_grid(p, &grid)) return 1;
  } else {
    const long M = (long)p.B * p.Ho * p.Wo;
    const int ntiles = r.family == CF_F32 ? (p.Cout + r.bn - 1) / r.bn : cout_padded(p.Cout) / r.bn;
    grid = (unsigned)(((M + r.bm - 1) / r.bm) * ntiles * sk);
  }
  (p.trace != nullptr && r.launch_traced != nullptr ? r.launch_traced : r.launch)(dev, grid, stream);
  if (sk > 1) launch_split_reduce(p, dev, stream);
  ODT_HIP(hipGetLastError());
  return 0;
}

size_t conv_split_partial_bytes(const ConvParams& p) {
  const int fam = conv_variant_row(p.variant).family;
  return (fam == CF_SPLIT3 || fam == CF_H2) && p.splitk > 1 ? (size_t)p.splitk * p.B * p.Ho * p.Wo * cout_padded(p.Cout) * sizeof(float) : 0;
}

// f32 weights [Cout][K] times a per-k gate (the exact-f32 kernel's form of the folded gate)
__global__ void __launch_bounds__(256) scale_weights_kernel(const float* __restrict__ wt, const float* __restrict__ kscale, long total, int K,
                                                            float* __restrict__ out) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < total) out[i] = wt[i] * kscale[(int)(i % K)];
}

int conv_scale_weights(const float* wt, const float* kscale, int Cout, int K, float* out, hipStream_t stream) {
  const long total = (long)Cout * K;
  hipLaunchKernelGGL(scale_weights_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, wt, kscale, total, K, out);
  ODT_HIP(hipGetLastError());
  return 0;
}

int conv_make_split_weights(const ConvParams& p, void* img_dev, hipStream_t stream, const float* wt_src, const float* kscale) {
  const float* src = wt_src != nullptr ? wt_src : p.wt;
  ODT_CHECK(kscale == nullptr || (p.kh == 1 && p.kw == 1 && p.in2 == nullptr), "conv_make_split_weights: a folded gate belongs to a single-source 1x1 conv");
  const ConvKernelRow& r = conv_variant_row(p.variant);
  const int bn = r.bn;
  const int K = conv_k(p);
  ODT_CHECK(r.launch != nullptr && r.family != CF_F32 && K % 32 == 0,
            "conv_make_split_weights: Cout % 64 == 0, K % 32 == 0 and a chosen kernel family required");
  if (r.family == CF_H2) {
    ODT_CHECK(kscale == nullptr && wt_src == nullptr, "conv_make_split_weights: the fp16x2 image takes the conv's own weights");
    return conv_make_h2_weights(p, img_dev, stream);
  }
  if (r.family == CF_SPLIT3) {
    const long total = (long)cout_padded(p.Cout) * (K >> 4) * 2;
    hipLaunchKernelGGL(split_weights3_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, src, p.Cout, K,
                       bn, p.kh * p.kw, p.Cin, (unsigned short*)img_dev, kscale);
  } else {
    const long total = (long)cout_padded(p.Cout) * (K >> 3);
    hipLaunchKernelGGL(split_weights_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, src, p.Cout, K,
                       bn, 32, (unsigned short*)img_dev, kscale);
  }
  ODT_HIP(hipGetLastError());
  return 0;
}

void conv_attach_weights(ConvParams& p, const void* img) {
  p.wt_split = img;
  if (conv_variant_row(p.variant).family == CF_H2) p.h2_chinv = conv_h2_chinv(img, p.Cout, conv_k(p));
}

}  // namespace odt
