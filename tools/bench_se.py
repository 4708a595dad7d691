#!/usr/bin/env python
"""The version-6 (SE-ResNet-101) detector step on one MI355X next to the same weights without squeeze-excitation.

python tools/bench_se.py [--batch 8] [--height 1080] [--width 1920] [--topk 300] [--steps 10] [--rounds 3]
  Multi graph, --rotate resident uint8 batches taken in turn, device-synchronised timing after a warm-up (as bench.py):
  the version-6 handle and a handle of the SAME weights with use_se=False (undilated, class-agnostic) are timed in
  alternating blocks of --steps steps inside one process.  Prints the step times, their difference, and the byte count of
  what SE adds to a step, computed here from the plan's shapes, over the project's measured copy rate.
python tools/bench_se.py --only v6 --steps 3
  Just the version-6 handle: the program to put behind `rocprofv3 --kernel-trace --stats --` for the per-kernel times of
  channel_sum_kernel / resnet_se_reduce_kernel / resnet_se_expand_kernel / resnet_se_apply_kernel.
One JSON line at the end."""
import argparse, copy, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

COPY_RATE = 6.29e12      # bytes/s, the project's measured device copy rate


def se_bytes(layers_se, layers_plain, B):
  """Bytes per step that the SE graph moves on top of the plain one, from the conv shapes of the two plans
  (profile_layers: name, flops, ms, (M, N, K)).  Per bottleneck with M pixels of the batch and width ch:
    pool            read of t2                                   M * ch * 4
    apply           y read + shortcut read + out write           3 * M * 4 ch * 4
    less            the residual read conv3's epilogue no longer does (identity blocks)   M * 4 ch * 4
    lost fusions    t2 written and read back where the plain plan folds conv3 into conv2's kernel   2 * M * ch * 4
                    the shortcut tensor written and read back at the stage entries (plain plan: one K-concatenated GEMM;
                    its read is the apply step's shortcut read, counted above)           M * 4 ch * 4"""
  plain = {n.split("[")[0]: n for n, _, _, _ in layers_plain}
  out = {"pool": 0, "apply_three_passes": 0, "less_conv3_residual_read": 0, "lost_tail_fusion_t2_round_trip": 0,
         "lost_entry_fusion_shortcut_write": 0, "blocks": 0}
  for name, _, _, (M, N, K) in layers_se:
    base = name.split("[")[0]
    if not base.endswith("/conv3"):
      continue
    pre = base[:-len("/conv3")]
    out["blocks"] += 1
    out["pool"] += M * K * 4
    out["apply_three_passes"] += 3 * M * N * 4
    if pre + "/conv3+shortcut" in plain:
      out["lost_entry_fusion_shortcut_write"] += M * N * 4
    else:
      out["less_conv3_residual_read"] -= M * N * 4
    if (pre + "/conv2+conv3") in plain:
      out["lost_tail_fusion_t2_round_trip"] += 2 * M * K * 4
  out["total"] = sum(v for k, v in out.items() if k != "blocks")
  out["apply_net_of_residual"] = out["apply_three_passes"] + out["less_conv3_residual_read"]
  return out


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--batch", type=int, default=8)
  ap.add_argument("--height", type=int, default=1080)
  ap.add_argument("--width", type=int, default=1920)
  ap.add_argument("--topk", type=int, default=300)
  ap.add_argument("--steps", type=int, default=10)
  ap.add_argument("--warmup", type=int, default=2)
  ap.add_argument("--rounds", type=int, default=3, help="alternations of (v6 block, plain block)")
  ap.add_argument("--rotate", type=int, default=4)
  ap.add_argument("--only", default="", choices=["", "v6", "plain"])
  ap.add_argument("--device", type=int, default=0)
  a = ap.parse_args()
  import torch
  from object_detection_tracking_amd import models
  from object_detection_tracking_amd._lib import ODT_DTYPE_U8
  from object_detection_tracking_amd.config import make_config
  from object_detection_tracking_amd.weights import synthetic_frames, synthetic_weights
  B, H, W = a.batch, a.height, a.width
  cfg6 = make_config(version=6, rpn_test_post_nms_topk=a.topk, im_batch_size=B, max_size=max(H, W), short_edge_size=min(H, W))
  cfg0 = copy.copy(cfg6); cfg0.use_se = False
  weights = synthetic_weights(cfg6, seed=0)
  frames = [synthetic_frames(B, H, W, seed=1234 + 77 * r) for r in range(max(1, a.rotate))]
  dev = [torch.from_numpy(f).cuda(a.device) for f in frames]
  torch.cuda.synchronize()
  legs = {}
  for tag, cfg in (("v6", cfg6), ("plain", cfg0)):
    if a.only and a.only != tag:
      continue
    m = models.get_model(cfg, a.device, weights=weights, is_multi=True)
    e = m.engine(B, H, W)
    e.forward_device_async(dev[0].data_ptr(), ODT_DTYPE_U8); e.synchronize()      # bring-up: the range guard's comparison
    legs[tag] = (m, e, [0])

  def run(tag, n):
    m, e, k = legs[tag]
    for _ in range(n):
      e.forward_device_async(dev[k[0] % len(dev)].data_ptr(), ODT_DTYPE_U8)
      k[0] += 1
    e.synchronize(); torch.cuda.synchronize()

  for tag in legs:
    run(tag, a.warmup)
  ms = {tag: [] for tag in legs}
  for _ in range(a.rounds):
    for tag in legs:
      t0 = time.perf_counter()
      run(tag, a.steps)
      ms[tag].append((time.perf_counter() - t0) / a.steps * 1e3)
  res = {"batch": B, "height": H, "width": W, "topk": a.topk, "steps": a.steps, "rounds": a.rounds,
         "step_ms_per_round": ms, "step_ms": {t: float(np.median(v)) for t, v in ms.items()}}
  for tag, (m, e, _) in legs.items():
    d = e.describe()
    res[tag] = {"fps": B * 1e3 / res["step_ms"][tag], "detections_last": int(e.read_outputs(False, False)[3].sum()),
                "conv_launches": d["conv_launches"], "fp16x2_split_launches": d["fp16x2_split_launches"],
                "bottleneck_tails_fused": d["bottleneck_tails_fused"], "se_blocks": d["se_blocks"],
                "se_blocks_conv1_on_fp16x2": d["se_blocks_conv1_on_fp16x2"], "range_guard": d.get("conv_split_family_auto", {}).get("chosen")}
  print("step ms per round: %s" % json.dumps(ms))
  if len(legs) == 2:
    diff = res["step_ms"]["v6"] - res["step_ms"]["plain"]
    by = se_bytes(legs["v6"][1].profile_layers(), legs["plain"][1].profile_layers(), B)
    res["se_minus_plain_ms"] = diff
    res["se_bytes_per_step"] = by
    res["se_bytes_over_copy_rate_ms"] = by["total"] / COPY_RATE * 1e3
    res["apply_bytes_over_copy_rate_ms"] = by["apply_three_passes"] / COPY_RATE * 1e3
    print("v6 %.3f ms/step (%.1f FPS)   plain %.3f ms/step (%.1f FPS)   difference %.3f ms" %
          (res["step_ms"]["v6"], res["v6"]["fps"], res["step_ms"]["plain"], res["plain"]["fps"], diff))
    print("SE additions per step, from shapes: %s" % json.dumps(by))
    print("  = %.2f GB -> %.2f ms at the measured copy rate of %.2f TB/s (apply passes alone: %.2f GB, %.2f ms)" %
          (by["total"] / 1e9, res["se_bytes_over_copy_rate_ms"], COPY_RATE / 1e12, by["apply_three_passes"] / 1e9,
           res["apply_bytes_over_copy_rate_ms"]))
  for m, e, _ in legs.values():
    m.close()
  print(json.dumps(res), flush=True)


if __name__ == "__main__":
  main()
