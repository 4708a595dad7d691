#!/usr/bin/env python
"""The detector step of the backbones the plan can build, on one MI355X: ResNet-101 (the default), ResNeXt-101 32x4d
(--use_resnext, [3,4,23,3]), ResNet-18 and ResNet-34 (--resnet18 / --resnet34), and ResNet-101 without dilations plain and with
--use_deformable (a deformable group3/block0; the reference graph does not build with dilations).

python tools/bench_backbones.py [--batch 8] [--height 1080] [--width 1920] [--topk 300] [--steps 10] [--warmup 2]
  One child process per backbone (a fresh runtime each; nothing of one handle is resident under the next).  Multi graph,
  --rotate resident uint8 batches taken in turn, device-synchronised timing after a warm-up (as bench.py).  Synthetic
  weights of seed 0.  For ResNeXt a second, profiled pass times every launch of the 32-group 3x3 conv (csrc/conv_group.hip)
  and prints the mean next to two floors computed here from the shapes: the bytes of its two tensors over the project's
  measured copy rate, and its f32 products over the measured rate of the exact-f32 MFMA.  For the deformable R101 a profiled
  pass times conv2_offset and the deformable conv (csrc/conv_deform.hip) next to the latter's product floor.
  Without --backbones the four block kinds run (r101, resnext101, resnet34, resnet18), as before the deformable rows.
python tools/bench_backbones.py --backbones r101_nodil,r101_deformable
  Only these, in this order, in one run: profiles/backbones_deformable_b8_1080p.txt.
python tools/bench_backbones.py --only resnext101 --steps 3
  Just that handle in this process: the program to put behind `rocprofv3 --kernel-trace --stats --` for per-kernel times.
python tools/bench_backbones.py --backbones r101,r50_gn,r101_gn
  The GroupNorm detectors (--use_gn) beside the BatchNorm R101, in one run: profiles/backbones_gn_b8_1080p.txt.  A profiled pass
  times the GroupNorm launches (csrc/group_norm.hip: statistics, finalize, apply per layer) and prints their share of the step
  next to the byte floor that describe() computes from the plan's own tensors -- every layer reads its conv output twice and
  writes it once, the block tails and the FPN sums read a residual on top -- over the measured copy rate.
python tools/bench_backbones.py --backbones r101,r101_convhead,r50_gn,r50_gn_convhead,r101_gn,r101_gn_convhead
  The 4-conv + FC box head (--use_conv_frcnn_head, conv_frcnn_head_dim 256) next to its 2-FC counterparts, in one run:
  profiles/backbones_convhead_b8_1080p.txt.  A profiled pass times the four head convs (fastrcnn/conv0..3: 3x3 over B x topk RoIs
  of 7 x 7) against their FLOP at the sustained rate of the fp16x2 kernels, and under --use_gn the four ROI GroupNorms
  (csrc/group_norm_roi.hip: one launch, one pass each) against the byte floor describe() computes from the plan's own tensors --
  one read and one write -- over the measured copy rate.
python tools/bench_backbones.py --graph single --batch 1 --backbones r101,r101_relation [--topk 1000]
  The relation-network box head (--add_relation_nn: RM_r1 behind fc6, RM_r2 behind fc7) next to the plain 2-FC head on the
  single-image graph, in one run: profiles/relation_b1_1080p.txt.  A profiled pass times, per module, the geometric-bias kernel
  and the attention kernel (csrc/relation.hip) and the Q | K and output_linear GEMMs, each next to a floor from the plan's own
  shapes: the two attention products (2 K^2 D + 32 K^2 D FLOP) at the exact-f32 MFMA rate, the GEMMs at the rate the fp16x2
  kernels sustain, the bias kernel's K^2 (64 tanh + 1280 FMA) at one v_fma_f32 per lane and clock, a tanh counted as 8 of them
  (an exp and a reciprocal at quarter rate).
python tools/bench_backbones.py --backbones r101,r101_att [--topk 1000]
  The attention branch of the box head (--use_att_frcnn_head) next to the plain 2-FC head, two rows that differ in the flag alone,
  in one run: profiles/att_head_b8_1080p.txt.  A profiled pass times the three launches of the branch: att_pool and att_add
  (csrc/att_head.hip) each next to its byte floor -- one read of the RoI features and one write of [R,C]; two reads and one write
  of [R,D]; their sum is describe()'s att_head_floor_bytes -- over the measured copy rate, and fastrcnn/att_trans next to its FLOP
  at the rate the fp16x2 kernels sustain.  The fp16x2 launch counts of the two rows say whether att_trans runs on those kernels.
One JSON line per backbone, and one with all of them at the end."""
import argparse, json, os, subprocess, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

COPY_RATE = 6.29e12      # bytes/s, the project's measured device copy rate
F32_MFMA_RATE = 155e12   # FLOP/s, v_mfma_f32_16x16x4_f32 back to back on every SIMD
H2_RATE = 341e12         # FLOP/s of f32 work the fp16x2 conv kernels sustain over the R101 step (README.md)
VEC_FMA_RATE = 256 * 64 * 2.4e9      # v_fma_f32 per second: 256 CUs x 64 lanes x 2.4 GHz
TANH_FMA_SLOTS = 8       # issue slots of a tanhf counted in v_fma_f32: v_exp_f32 + v_rcp_f32 at quarter rate, nothing else
BACKBONES = {"r101": {}, "resnext101": dict(use_resnext=True), "resnet34": dict(resnet34=True), "resnet18": dict(resnet18=True),
             "r101_nodil": dict(use_dilations=False), "r101_deformable": dict(use_dilations=False, use_deformable=True),
             "r50_gn": dict(resnet50=True, use_gn=True), "r101_gn": dict(use_gn=True),
             "r101_convhead": dict(use_conv_frcnn_head=True), "r50_gn_convhead": dict(resnet50=True, use_gn=True, use_conv_frcnn_head=True),
             "r101_gn_convhead": dict(use_gn=True, use_conv_frcnn_head=True),
             "r101_relation": dict(add_relation_nn=True), "r101_att": dict(use_att_frcnn_head=True)}
DEFAULT = ("r101", "resnext101", "resnet34", "resnet18")   # what a run without --backbones measures (profiles/backbones_b8_1080p.txt)


def group_conv_shapes(cfg, B, H, W):
  """[(C, H, W, Ho, Wo, stride, dil)] of the plan's grouped convs, by the plan's rules: the frame padded to a multiple of
  32, a quarter of it after conv0 + pool0, 'SAME' at stride 2 on the stage entries."""
  h, w = -(-H // 32) * 32 // 4, -(-W // 32) * 32 // 4
  out = []
  for g, (ch, cnt) in enumerate(zip((64, 128, 256, 512), cfg.resnet_num_block)):
    for i in range(cnt):
      stride = 2 if (i == 0 and g > 0) else 1
      dil = 2 if (g == 3 and cfg.use_dilations and i >= cnt - 3) else 1
      ho, wo = -(-h // stride), -(-w // stride)
      out.append((2 * ch, h, w, ho, wo, stride, dil))
      h, w = ho, wo
  return out


def deform_conv_shapes(cfg, H, W):
  """[(C, Ho, Wo)] of the plan's deformable convs, by the plan's rules: the stride-2 bottleneck that opens group 1-3 where
  the group has at most three blocks; C is the block's conv2 width, Ho x Wo its output map."""
  h, w = -(-H // 32) * 32 // 4, -(-W // 32) * 32 // 4
  out = []
  for g, (ch, cnt) in enumerate(zip((64, 128, 256, 512), cfg.resnet_num_block)):
    if g > 0:
      h, w = -(-h // 2), -(-w // 2)
      if cfg.use_deformable and cnt <= 3:
        out.append((ch, h, w))
  return out


def child(a, name):
  import torch
  from object_detection_tracking_amd import models
  from object_detection_tracking_amd._lib import ODT_DTYPE_U8
  from object_detection_tracking_amd.config import make_config
  from object_detection_tracking_amd.weights import synthetic_frames, synthetic_weights
  B, H, W = a.batch, a.height, a.width
  cfg = make_config(rpn_test_post_nms_topk=a.topk, im_batch_size=B, max_size=max(H, W), short_edge_size=min(H, W), **BACKBONES[name])
  weights = synthetic_weights(cfg, seed=0)
  frames = [synthetic_frames(B, H, W, seed=1234 + 77 * r) for r in range(max(1, a.rotate))]
  dev = [torch.from_numpy(f).cuda(a.device) for f in frames]
  torch.cuda.synchronize()
  m = models.get_model(cfg, a.device, weights=weights, is_multi=a.graph == "multi")
  e = m.engine(B, H, W)
  e.forward_device_async(dev[0].data_ptr(), ODT_DTYPE_U8); e.synchronize()      # bring-up: the range guard's comparison
  k = [0]

  def run(n):
    for _ in range(n):
      e.forward_device_async(dev[k[0] % len(dev)].data_ptr(), ODT_DTYPE_U8)
      k[0] += 1
    e.synchronize(); torch.cuda.synchronize()

  run(a.warmup)
  ms = []
  for _ in range(a.rounds):
    t0 = time.perf_counter()
    run(a.steps)
    ms.append((time.perf_counter() - t0) / a.steps * 1e3)
  d = e.describe()
  res = {"backbone": name, "blocks": list(cfg.resnet_num_block), "block_kind": d["block_kind"], "batch": B, "height": H, "width": W,
         "topk": a.topk, "step_ms_per_round": ms, "step_ms": float(np.median(ms)), "fps": B * 1e3 / float(np.median(ms)),
         "detections_last": int(e.read_outputs(False, False)[3].sum()), "conv_launches": d["conv_launches"],
         "fp16x2_split_launches": d["fp16x2_split_launches"], "bottleneck_tails_fused": d["bottleneck_tails_fused"],
         "group_conv_launches": d["group_conv_launches"], "range_guard": d.get("conv_split_family_auto", {}).get("chosen")}
  if d["group_conv_launches"] > 0:
    e.profile(True)
    run(a.steps)
    dp = e.describe()
    e.profile(False)
    shapes = group_conv_shapes(cfg, B, H, W)
    assert len(shapes) == d["group_conv_launches"], (len(shapes), d["group_conv_launches"])
    by = sum(4.0 * B * C * (h * w + ho * wo) for C, h, w, ho, wo, _, _ in shapes)
    fl = sum(2.0 * B * ho * wo * C * 9 * (C // 32) for C, h, w, ho, wo, _, _ in shapes)
    per_fwd = dp["group_conv_profiled_ms"] / max(1, dp["profiled_forwards"])
    res["group_conv"] = {"ms_per_step": per_fwd, "ms_per_launch": per_fwd / len(shapes), "bytes_per_step": by, "flop_per_step": fl,
                         "floor_ms_bytes_over_copy_rate": by / COPY_RATE * 1e3, "floor_ms_flop_over_f32_mfma_rate": fl / F32_MFMA_RATE * 1e3}
  if d.get("deform_conv_launches", 0) > 0:
    e.profile(True)
    run(a.steps)
    dp = e.describe()
    e.profile(False)
    shapes = deform_conv_shapes(cfg, H, W)      # R50 / R101 / R152: group3/block0 alone, C = 512 on the 1/32 map
    assert len(shapes) == d["deform_conv_launches"], (len(shapes), d["deform_conv_launches"])
    px = sum(B * ho * wo for _, ho, wo in shapes)
    fl = sum(2.0 * B * ho * wo * 9 * C * C for C, ho, wo in shapes)
    n = max(1, dp["profiled_forwards"])
    res["deform_conv"] = {"offset_ms_per_step": dp["deform_offset_profiled_ms"] / n, "conv_ms_per_step": dp["deform_conv_profiled_ms"] / n,
                          "output_pixels": px, "flop_per_step": fl, "offset_flop_per_step": sum(2.0 * B * ho * wo * 9 * C * 18 for C, ho, wo in shapes),
                          "floor_ms_flop_over_f32_mfma_rate": fl / F32_MFMA_RATE * 1e3}
  if d.get("group_norms", 0) > 0:
    e.profile(True)
    run(a.steps)
    dp = e.describe()
    e.profile(False)
    per_fwd = dp["group_norm_profiled_ms"] / max(1, dp["profiled_forwards"])
    res["group_norm"] = {"layers": d["group_norms"], "ms_per_step": per_fwd, "share_of_step": per_fwd / res["step_ms"],
                         "bytes_per_step": d["group_norm_floor_bytes"], "floor_ms_bytes_over_copy_rate": d["group_norm_floor_bytes"] / COPY_RATE * 1e3}
  res["box_head"] = d["box_head"]
  if d["box_head"] == "4conv1fc":
    e.profile(True)
    run(a.steps)
    dp = e.describe()
    layers = [(nm, fl, ms) for nm, fl, ms, _ in e.profile_layers() if nm.startswith("fastrcnn/conv")]
    e.profile(False)
    n = max(1, dp["profiled_forwards"])
    assert len(layers) == 4, layers
    fl = sum(f for _, f, _ in layers)
    res["head_convs"] = {"layers": [nm for nm, _, _ in layers], "ms_per_step": sum(ms for _, _, ms in layers) / n, "flop_per_step": fl,
                         "floor_ms_flop_over_fp16x2_rate": fl / H2_RATE * 1e3}
    if dp["roi_group_norms"] > 0:
      res["roi_group_norm"] = {"layers": dp["roi_group_norms"], "ms_per_step": dp["roi_group_norm_profiled_ms"] / n,
                               "bytes_per_step": dp["roi_group_norm_floor_bytes"],
                               "floor_ms_bytes_over_copy_rate": dp["roi_group_norm_floor_bytes"] / COPY_RATE * 1e3}
  if d.get("relation_modules", 0) > 0:
    e.profile(True)
    run(a.steps)
    dp = e.describe()
    layers = {nm.split("[")[0]: (fl, ms) for nm, fl, ms, _ in e.profile_layers() if "/RM_r" in nm}
    e.profile(False)
    n = max(1, dp["profiled_forwards"])
    K, D = a.topk, int(cfg.fpn_frcnn_fc_head_dim)
    att_fl = B * (2.0 * K * K * D + 32.0 * K * K * D)
    geo_fma, geo_tanh = B * K * K * (4 * 64 + 64 * 16), B * K * K * 64
    res["relation"] = []
    for i, scope in enumerate(("fastrcnn/RM_r1", "fastrcnn/RM_r2")):
      qk, ol = layers[scope + "/query_key_linear"], layers[scope + "/output_linear"]
      res["relation"].append({
          "module": scope, "geo_ms": dp["relation_geo_profiled_ms"][i] / n, "geo_fma": geo_fma, "geo_tanh": geo_tanh,
          "geo_floor_ms": (geo_fma + TANH_FMA_SLOTS * geo_tanh) / VEC_FMA_RATE * 1e3,
          "attention_ms": dp["relation_attention_profiled_ms"][i] / n, "attention_flop": att_fl,
          "attention_floor_ms": att_fl / F32_MFMA_RATE * 1e3,
          "qk_ms": qk[1] / n, "qk_flop": qk[0], "qk_floor_ms": qk[0] / H2_RATE * 1e3,
          "output_linear_ms": ol[1] / n, "output_linear_flop": ol[0], "output_linear_floor_ms": ol[0] / H2_RATE * 1e3})
  if d.get("att_frcnn_head", 0):
    e.profile(True)
    run(a.steps)
    dp = e.describe()
    trans = [(fl, ms) for nm, fl, ms, _ in e.profile_layers() if nm.split("[")[0] == "fastrcnn/att_trans"]
    e.profile(False)
    n = max(1, dp["profiled_forwards"])
    assert len(trans) == 1, trans
    R, C, D = B * a.topk, int(cfg.fpn_num_channel), int(cfg.fpn_frcnn_fc_head_dim)
    pool_by, add_by = 4.0 * R * C * (49 + 1), 12.0 * R * D
    assert pool_by + add_by == dp["att_head_floor_bytes"], (pool_by, add_by, dp["att_head_floor_bytes"])
    pool_ms, trans_ms, add_ms = (t / n for t in dp["att_head_profiled_ms"])
    assert abs(trans_ms - trans[0][1] / n) < 1e-9, (trans_ms, trans[0][1] / n)
    res["att_head"] = {"pool_ms": pool_ms, "pool_bytes": pool_by, "pool_floor_ms": pool_by / COPY_RATE * 1e3,
                       "add_ms": add_ms, "add_bytes": add_by, "add_floor_ms": add_by / COPY_RATE * 1e3,
                       "att_trans_ms": trans_ms, "att_trans_flop": trans[0][0], "att_trans_floor_ms": trans[0][0] / H2_RATE * 1e3}
  m.close()
  print(json.dumps(res), flush=True)
  return res


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--batch", type=int, default=8)
  ap.add_argument("--height", type=int, default=1080)
  ap.add_argument("--width", type=int, default=1920)
  ap.add_argument("--topk", type=int, default=300)
  ap.add_argument("--steps", type=int, default=10)
  ap.add_argument("--warmup", type=int, default=2)
  ap.add_argument("--rounds", type=int, default=3)
  ap.add_argument("--rotate", type=int, default=4)
  ap.add_argument("--only", default="", choices=[""] + sorted(BACKBONES))
  ap.add_argument("--backbones", default="", help="comma-separated subset of %s (default: %s)" % (", ".join(BACKBONES), ",".join(DEFAULT)))
  ap.add_argument("--device", type=int, default=0)
  ap.add_argument("--graph", default="multi", choices=["multi", "single"], help="Mask_RCNN_FPN_multi (default) or the single-image Mask_RCNN_FPN")
  a = ap.parse_args()
  if a.only:
    child(a, a.only)
    return
  out = {}
  names = [n for n in a.backbones.split(",") if n] or list(DEFAULT)
  for name in names:
    if name not in BACKBONES:
      sys.exit("unknown backbone %s" % name)
    cmd = [sys.executable, os.path.abspath(__file__), "--only", name] + \
        [x for k in ("batch", "height", "width", "topk", "steps", "warmup", "rounds", "rotate", "device", "graph") for x in ("--" + k, str(getattr(a, k)))]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
    if r.returncode != 0:
      sys.exit("%s: child exited with %d" % (name, r.returncode))
    res = json.loads(r.stdout.strip().splitlines()[-1])
    out[name] = res
    line = "%-16s %s %-12s %8.3f ms/step  %7.1f FPS  (%d conv launches, %d fused tails)" % (
        name, res["blocks"], res["block_kind"], res["step_ms"], res["fps"], res["conv_launches"], res["bottleneck_tails_fused"])
    if any("att_head" in r for r in out.values()) or "r101_att" in names:
      line += "  [%d on fp16x2]" % res["fp16x2_split_launches"]
    print(line)
    if "group_conv" in res:
      g = res["group_conv"]
      print("            grouped 3x3: %d launches, %.3f ms/step measured, %.4f ms/launch;  floors from shapes: %.2f GB -> %.3f ms at "
            "%.2f TB/s, %.0f GFLOP -> %.3f ms at %.0f TF" % (res["group_conv_launches"], g["ms_per_step"], g["ms_per_launch"],
            g["bytes_per_step"] / 1e9, g["floor_ms_bytes_over_copy_rate"], COPY_RATE / 1e12, g["flop_per_step"] / 1e9,
            g["floor_ms_flop_over_f32_mfma_rate"], F32_MFMA_RATE / 1e12))
    if "deform_conv" in res:
      g = res["deform_conv"]
      print("            deformable conv2: %.3f ms/step measured (+ conv2_offset %.3f ms);  floor from the shape: %.1f GFLOP -> %.3f ms "
            "at %.0f TF" % (g["conv_ms_per_step"], g["offset_ms_per_step"], g["flop_per_step"] / 1e9, g["floor_ms_flop_over_f32_mfma_rate"],
            F32_MFMA_RATE / 1e12))
    if "group_norm" in res:
      g = res["group_norm"]
      print("            GroupNorm: %d layers, %.3f ms/step measured in a profiled pass (%.0f %% of the step);  floor from the plan's tensors: "
            "%.1f GB -> %.3f ms at %.2f TB/s" % (g["layers"], g["ms_per_step"], 100.0 * g["share_of_step"], g["bytes_per_step"] / 1e9,
            g["floor_ms_bytes_over_copy_rate"], COPY_RATE / 1e12))
    if "head_convs" in res:
      g = res["head_convs"]
      print("            4-conv head: %s, %.3f ms/step measured in a profiled pass;  %.2f TFLOP -> %.3f ms at the %.0f TF the fp16x2 "
            "kernels sustain (measured / floor %.2f)" % (" ".join(n.split("/")[-1] for n in g["layers"]), g["ms_per_step"], g["flop_per_step"] / 1e12,
            g["floor_ms_flop_over_fp16x2_rate"], H2_RATE / 1e12, g["ms_per_step"] / g["floor_ms_flop_over_fp16x2_rate"]))
    if "roi_group_norm" in res:
      g = res["roi_group_norm"]
      print("            ROI GroupNorm: %d layers, %.3f ms/step measured;  floor from the plan's tensors (one read + one write): %.2f GB -> "
            "%.3f ms at %.2f TB/s (measured / floor %.2f)" % (g["layers"], g["ms_per_step"], g["bytes_per_step"] / 1e9,
            g["floor_ms_bytes_over_copy_rate"], COPY_RATE / 1e12, g["ms_per_step"] / g["floor_ms_bytes_over_copy_rate"]))
    for g in res.get("relation", []):
      print("            %s: bias %.3f ms (floor %.3f: %.0f M tanh + %.0f M FMA), attention %.3f ms (floor %.3f: %.1f GFLOP at %.0f TF), "
            "Q|K %.3f ms (floor %.3f), output_linear %.3f ms (floor %.3f: %.1f GFLOP at %.0f TF)" % (
                g["module"].split("/")[-1], g["geo_ms"], g["geo_floor_ms"], g["geo_tanh"] / 1e6, g["geo_fma"] / 1e6, g["attention_ms"],
                g["attention_floor_ms"], g["attention_flop"] / 1e9, F32_MFMA_RATE / 1e12, g["qk_ms"], g["qk_floor_ms"],
                g["output_linear_ms"], g["output_linear_floor_ms"], g["output_linear_flop"] / 1e9, H2_RATE / 1e12))
    if "att_head" in res:
      g = res["att_head"]
      print("            attention branch (profiled pass): att_pool %.4f ms (floor %.4f: %.1f MB at %.2f TB/s, measured / floor %.2f), "
            "att_trans %.4f ms (floor %.4f: %.2f GFLOP at %.0f TF, measured / floor %.2f), att_add %.4f ms (floor %.4f: %.1f MB, "
            "measured / floor %.2f)" % (g["pool_ms"], g["pool_floor_ms"], g["pool_bytes"] / 1e6, COPY_RATE / 1e12, g["pool_ms"] / g["pool_floor_ms"],
                                        g["att_trans_ms"], g["att_trans_floor_ms"], g["att_trans_flop"] / 1e9, H2_RATE / 1e12,
                                        g["att_trans_ms"] / g["att_trans_floor_ms"], g["add_ms"], g["add_floor_ms"], g["add_bytes"] / 1e6,
                                        g["add_ms"] / g["add_floor_ms"]))
  print(json.dumps(out), flush=True)


if __name__ == "__main__":
  main()
