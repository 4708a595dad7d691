"""Weight ingest for the detector: Tensorpack-style ``.npz`` (the only format
the reference can load without TensorFlow, reference
obj_detect_tracking.py:417-435) and a seeded synthetic generator that emits
exactly the same variable names / layouts:

  conv ``W``  : HWIO  [kh, kw, Cin, Cout]        (reference nn.py:350,367)
  dense ``W`` : [in, out], ``in`` flattened NCHW (reference nn.py:736-757)
  BN          : gamma, beta, mean/EMA, variance/EMA (reference nn.py:1821-1839)

No network and no checkpoints ship with the reference, so benchmarks and
parity tests use :func:`synthetic_weights` (random-init weights of the real
architecture).
"""
from __future__ import annotations

import numpy as np


def _strip(name):
  return name[:-2] if name.endswith(":0") else name


def load_npz(path):
  """Load a Tensorpack/zoo ``.npz`` into {name: float32 array} (names without
  the ``:0`` suffix the reference adds back, obj_detect_tracking.py:419-420)."""
  with np.load(path) as z:
    return {_strip(k): np.asarray(z[k]) for k in z.files}


def backbone_block_kind(config):
  """0 bottleneck | 1 basic block (use_basic_block) | 2 ResNeXt-32x4d (use_resnext, which takes precedence: nn.py:864-868)."""
  if getattr(config, "use_resnext", False):
    return 2
  return 1 if getattr(config, "use_basic_block", False) else 0


def deformable_groups(config):
  """The groups whose block 0 is deformable under --use_deformable (reference nn.py:469-485, 574-585): a resnet_bottleneck of
  stride 2 (block 0 of group 1, 2 or 3) that is among the last three blocks of its group.  [3, 4, 23, 3] -> [3]."""
  if not getattr(config, "use_deformable", False) or backbone_block_kind(config) != 0:
    return []
  return [g for g in (1, 2, 3) if 1 <= config.resnet_num_block[g] <= 3]


def group_norm_scopes(config):
  """The GroupNorm scopes of a --use_gn graph in execution order (reference nn.py:81-108, 859-862, 987-1009): X/gn behind every
  backbone conv X that carries X/bn without the flag, fpn/gn_cN behind the lateral and fpn/gn_pN behind the posthoc convs.
  [] without the flag."""
  if not getattr(config, "use_gn", False):
    return []
  out = []
  for scope, _, _, _, has_bn, _ in backbone_conv_specs(config):
    if has_bn:
      out.append(scope + "/gn")
    elif scope.startswith("fpn/lateral_1x1_") or scope.startswith("fpn/posthoc_3x3_"):
      out.append("fpn/gn_" + scope[16:])
  return out


def group_norm_variables(config):
  """Names of the gamma / beta variables a --use_gn graph needs, in execution order."""
  return [s + "/" + v for s in group_norm_scopes(config) for v in ("gamma", "beta")]


def conv_head_variables(config):
  """Names of the variables a --use_conv_frcnn_head graph needs on top of the output layers, in execution order (reference
  conv_frcnn_head, models.py:1110-1124): fastrcnn/conv{k}/{W,b}, under use_gn each followed by fastrcnn/gn{k}/{gamma,beta},
  then fastrcnn/fc/{W,b}.  [] without the flag."""
  if not getattr(config, "use_conv_frcnn_head", False):
    return []
  out = []
  for k in range(4):
    out += ["fastrcnn/conv%d/W" % k, "fastrcnn/conv%d/b" % k]
    if getattr(config, "use_gn", False):
      out += ["fastrcnn/gn%d/gamma" % k, "fastrcnn/gn%d/beta" % k]
  return out + ["fastrcnn/fc/W", "fastrcnn/fc/b"]


RELATION_SCOPES = ("fastrcnn/RM_r1", "fastrcnn/RM_r2")
RELATION_VARIABLES = ("geo_emb/W", "geo_emb/b", "geo_conv/W", "geo_conv/b", "query_linear/W", "key_linear/W", "output_linear/W")


# standard deviations of the synthetic relation variables (query / key / output: times 1 / sqrt(fan-in))
RELATION_SCALES = {"geo_emb/W": 0.5, "geo_emb/b": 0.1, "geo_conv/W": 0.25, "geo_conv/b": 0.1, "query_linear/W": 1.0,
                   "key_linear/W": 1.0, "output_linear/W": 1.0}


def relation_variables(config):
  """Names of the variables an --add_relation_nn graph needs on top of the 2-FC head, in execution order (reference
  relation_network, nn.py:115-190, under fastrcnn/RM_r1 and fastrcnn/RM_r2: models.py:1044-1054): geo_emb/{W [4,64], b},
  geo_conv/{W [1,1,64,16], b}, query_linear/W and key_linear/W [D,D], output_linear/W [16 D,D].  [] without the flag."""
  if not getattr(config, "add_relation_nn", False):
    return []
  return [s + "/" + v for s in RELATION_SCOPES for v in RELATION_VARIABLES]


def att_head_variables(config):
  """Names of the variables a --use_att_frcnn_head graph needs on top of its box head, in the reference's order of creation
  (fastrcnn_2fc_head, models.py:1064-1089): fastrcnn/attention/{W [3,3,C,1], b [1]} -- the conv behind the one-channel softmax,
  which the graph owns and whose values cannot reach the output -- and fastrcnn/att_trans/{W [C,dim], b [dim]}.  [] without the
  flag."""
  if not getattr(config, "use_att_frcnn_head", False):
    return []
  return ["fastrcnn/attention/W", "fastrcnn/attention/b", "fastrcnn/att_trans/W", "fastrcnn/att_trans/b"]


def backbone_conv_specs(config):
  """Yield (scope, kh, cin, cout, has_bn, has_bias) for every conv on the path,
  in execution order (reference nn.py:843-1014, models.py:979-1009); cin is W's third dimension -- the channels per
  group of a grouped conv.  A deformable block's conv2 has neither BN nor bias; its conv2_offset is not listed here
  (synthetic_weights draws it from a generator of its own)."""
  blocks = config.resnet_num_block
  kind = backbone_block_kind(config)
  deform = deformable_groups(config)
  yield ("conv0", 7, 3, 64, True, False)
  cin = 64
  for g, (feat, cnt) in enumerate(zip((64, 128, 256, 512), blocks)):
    for i in range(cnt):
      pre = "group%d/block%d" % (g, i)
      if kind == 1:       # resnet_basicblock (nn.py:439-456): a shortcut conv only where the width changes (not in group0)
        yield (pre + "/conv1", 3, cin, feat, True, False)
        yield (pre + "/conv2", 3, feat, feat, True, False)
        if cin != feat:
          yield (pre + "/convshortcut", 1, cin, feat, True, False)
        cin = feat
        continue
      if kind == 2:       # resnext_32x4d_bottleneck (nn.py:524-549): conv2 in 32 groups, W [3,3,2 feat / 32,2 feat]
        yield (pre + "/conv1", 1, cin, feat * 2, True, False)
        yield (pre + "/conv2", 3, feat * 2 // 32, feat * 2, True, False)
        yield (pre + "/conv3", 1, feat * 2, feat * 4, True, False)
      else:
        yield (pre + "/conv1", 1, cin, feat, True, False)
        yield (pre + "/conv2", 3, feat, feat, not (i == 0 and g in deform), False)
        yield (pre + "/conv3", 1, feat, feat * 4, True, False)
      if i == 0:
        yield (pre + "/convshortcut", 1, cin, feat * 4, True, False)
      cin = feat * 4
  ch = config.fpn_num_channel
  for i, c in enumerate((64, 128, 256, 512) if kind == 1 else (256, 512, 1024, 2048)):
    yield ("fpn/lateral_1x1_c%d" % (i + 2), 1, c, ch, False, True)
  for i in range(4):
    yield ("fpn/posthoc_3x3_p%d" % (i + 2), 3, ch, ch, False, True)
  na = len(config.anchor_ratios)
  yield ("rpn/conv0", 3, ch, ch, False, True)
  yield ("rpn/class", 1, ch, na, False, True)
  yield ("rpn/box", 1, ch, 4 * na, False, True)


def synthetic_weights(config, seed=0):
  """Seeded random-init weights with the reference's names and layouts.

  Distributions follow SURVEY.md section 8(d): He-init convs, BN close to
  identity (so activations stay O(1) through 101 layers), the last BN gamma of
  each block scaled by 0.12 (conv3/bn; conv2/bn of a basic block), RPN class bias +1 (so the top-K logits are
  positive and the multibatch zero-padding quirk does not starve the head), box-head ``class`` /
  ``box`` weights wide enough that several classes pass the 1e-4 score filter
  and boxes actually move.
  """
  rng = np.random.default_rng(seed)
  w = {}
  basic = backbone_block_kind(config) == 1
  # a deformable block's conv2 has no BN (nn.py:483-485): its four draws are made and dropped, so that every other variable
  # stays bit-identical to the weights of the same seed without the flag
  bn_less = {"group%d/block0/conv2" % g for g in deformable_groups(config)}
  # --use_gn: likewise every BN draw is made and dropped; the gn/{gamma,beta} variables come from a generator of their own
  use_gn = bool(getattr(config, "use_gn", False))

  def normal(shape, std):
    return (rng.standard_normal(shape, dtype=np.float32) * np.float32(std))

  for scope, k, cin, cout, has_bn, has_bias in backbone_conv_specs(config):
    fan_in = k * k * cin
    std = np.sqrt(2.0 / fan_in)
    if scope.startswith("fpn/lateral"):
      std = 0.35 * np.sqrt(1.0 / fan_in)
    if scope.startswith("fpn/posthoc"):
      std = 0.8 * np.sqrt(1.0 / fan_in)
    if scope in ("rpn/class", "rpn/box"):
      std = 0.05 if scope == "rpn/class" else 0.02
    w[scope + "/W"] = normal((k, k, cin, cout), std)
    if has_bias:
      b = normal((cout,), 0.02)
      if scope == "rpn/class":
        b = b + np.float32(1.0)
      w[scope + "/b"] = b
    if has_bn or scope in bn_less:
      bn = {}
      gamma = rng.uniform(0.9, 1.1, cout).astype(np.float32)
      if scope.endswith("/conv3") or (basic and scope.endswith("/conv2")):      # the block's last BN
        gamma *= np.float32(0.12)
      bn[scope + "/bn/gamma"] = gamma
      bn[scope + "/bn/beta"] = normal((cout,), 0.02)
      bn[scope + "/bn/mean/EMA"] = normal((cout,), 0.05)
      bn[scope + "/bn/variance/EMA"] = rng.uniform(0.8, 1.2, cout).astype(
          np.float32)
      if has_bn and not use_gn:
        w.update(bn)
  dim = config.fpn_frcnn_fc_head_dim
  ch = config.fpn_num_channel
  nc = config.num_class
  # --use_conv_frcnn_head: the four fc6 / fc7 draws are made and dropped (every other variable stays bit-identical to the weights
  # of the same seed without the flag); the head's own variables come from a generator of their own, below
  conv_head = bool(getattr(config, "use_conv_frcnn_head", False))
  fcs = {"fastrcnn/fc6/W": normal((ch * 49, dim), np.sqrt(2.0 / (ch * 49)))}
  fcs["fastrcnn/fc6/b"] = normal((dim,), 0.02)
  fcs["fastrcnn/fc7/W"] = normal((dim, dim), np.sqrt(2.0 / dim))
  fcs["fastrcnn/fc7/b"] = normal((dim,), 0.02)
  if not conv_head:
    w.update(fcs)
  w["fastrcnn/outputs/class/W"] = normal((dim, nc), 0.05)
  w["fastrcnn/outputs/class/b"] = normal((nc,), 0.02)
  if getattr(config, "add_mask", False):           # maskrcnn_up4conv_head (models.py:1173-1199)
    md = getattr(config, "mrcnn_head_dim", 256)
    cin = ch
    for k in range(4):
      w["maskrcnn/fcn%d/W" % k] = normal((3, 3, cin, md), np.sqrt(2.0 / (9 * cin)))
      w["maskrcnn/fcn%d/b" % k] = normal((md,), 0.02)
      cin = md
    w["maskrcnn/deconv/W"] = normal((2, 2, md, md), np.sqrt(2.0 / md))     # [kh, kw, out, in]
    w["maskrcnn/deconv/b"] = normal((md,), 0.02)
    w["maskrcnn/conv/W"] = normal((1, 1, md, nc - 1), np.sqrt(2.0 / md))
    w["maskrcnn/conv/b"] = normal((nc - 1,), 0.02)
  nb = 1 if getattr(config, "use_frcnn_class_agnostic", False) else nc   # models.py:1164
  w["fastrcnn/outputs/box/W"] = normal((dim, nb * 4), 0.01)
  w["fastrcnn/outputs/box/b"] = normal((nb * 4,), 0.002)
  if getattr(config, "use_se", False):
    # squeeze-excitation (version 6, nn.py:506-517) from a generator of its own: everything above is bit-identical to the
    # non-SE weights of the same seed.  Wide fc2 so that the gates spread over (0, 1) and a missing gate shows
    se_rng = np.random.default_rng([seed, 6])

    def se_normal(shape, std):
      return se_rng.standard_normal(shape, dtype=np.float32) * np.float32(std)

    for g, (feat, cnt) in enumerate(zip((64, 128, 256, 512), config.resnet_num_block)):
      for i in range(cnt):
        pre = "group%d/block%d" % (g, i)
        C, r = 4 * feat, feat // 4
        w[pre + "/fc1/W"] = se_normal((C, r), np.sqrt(2.0 / C))
        w[pre + "/fc1/b"] = se_normal((r,), 0.02)
        w[pre + "/fc2/W"] = se_normal((r, C), np.sqrt(2.0 / r))
        w[pre + "/fc2/b"] = se_normal((C,), 0.5)
  if deformable_groups(config):
    # --use_deformable (nn.py:469-485): conv2_offset of the deformable stage entries from a generator of its own.  Offsets of
    # a pixel or two (std 1.3 - 1.5 px, |max| 3.5 - 5 px on the synthetic frames): nearly every sample coordinate is fractional
    # and a good part of them clamps at the border of the small test maps
    d_rng = np.random.default_rng([seed, 7])
    for g in deformable_groups(config):
      C = (64, 128, 256, 512)[g]
      pre = "group%d/block0/conv2_offset" % g
      w[pre + "/W"] = d_rng.standard_normal((3, 3, C, 18), dtype=np.float32) * np.float32(1.5 * np.sqrt(1.0 / (9 * C)))
      w[pre + "/b"] = d_rng.standard_normal((18,), dtype=np.float32) * np.float32(0.5)
  if use_gn:
    # --use_gn (nn.py:81-108): gamma ~ U[0.9, 1.1], beta ~ N(0, 0.02); a block's last norm (conv3/gn) scaled by 0.25, so that the
    # residual branch neither vanishes nor swamps the shortcut behind a normalisation to unit variance
    g_rng = np.random.default_rng([seed, 8])
    chans = {s: c for s, _, _, c, _, _ in backbone_conv_specs(config)}
    for scope in group_norm_scopes(config):
      conv = scope[:-3] if scope.endswith("/gn") else ("fpn/lateral_1x1_" if scope[7] == "c" else "fpn/posthoc_3x3_") + scope[7:]
      C = chans[conv]
      gamma = g_rng.uniform(0.9, 1.1, C).astype(np.float32)
      if scope.endswith("/conv3/gn"):
        gamma *= np.float32(0.25)
      w[scope + "/gamma"] = gamma
      w[scope + "/beta"] = g_rng.standard_normal(C, dtype=np.float32) * np.float32(0.02)
  if conv_head:
    # --use_conv_frcnn_head (models.py:1110-1124): He-init 3x3 convs, biases N(0, 0.02), fc drawn as fc6 is; under use_gn
    # fastrcnn/gn{k} with gamma ~ U[0.9, 1.1], beta ~ N(0, 0.02)
    h_rng = np.random.default_rng([seed, 9])
    dc = int(getattr(config, "conv_frcnn_head_dim", 256))
    cin = ch
    for k in range(4):
      w["fastrcnn/conv%d/W" % k] = h_rng.standard_normal((3, 3, cin, dc), dtype=np.float32) * np.float32(np.sqrt(2.0 / (9 * cin)))
      w["fastrcnn/conv%d/b" % k] = h_rng.standard_normal((dc,), dtype=np.float32) * np.float32(0.02)
      if use_gn:
        w["fastrcnn/gn%d/gamma" % k] = h_rng.uniform(0.9, 1.1, dc).astype(np.float32)
        w["fastrcnn/gn%d/beta" % k] = h_rng.standard_normal(dc, dtype=np.float32) * np.float32(0.02)
      cin = dc
    w["fastrcnn/fc/W"] = h_rng.standard_normal((dc * 49, dim), dtype=np.float32) * np.float32(np.sqrt(2.0 / (dc * 49)))
    w["fastrcnn/fc/b"] = h_rng.standard_normal((dim,), dtype=np.float32) * np.float32(0.02)
  if getattr(config, "add_relation_nn", False):
    # --add_relation_nn (nn.py:115-190) from a generator of its own.  The scales make the attention informative on the synthetic
    # frames (tests/relation_reference.py asserts it on the reference alone): geo_conv spreads a[i,j,h] around zero, so that about
    # half of the pairs pass the ReLU and the rest sit at the log(1e-6) floor; query / key give logits of a few units over the
    # post-ReLU features (|h6|, |h7| ~ sqrt(D) on these weights), so that a softmax row is neither uniform nor one-hot;
    # output_linear keeps RM at the size of its input
    r_rng = np.random.default_rng([seed, 10])
    for scope in RELATION_SCOPES:
      w[scope + "/geo_emb/W"] = r_rng.standard_normal((4, 64), dtype=np.float32) * np.float32(RELATION_SCALES["geo_emb/W"])
      w[scope + "/geo_emb/b"] = r_rng.standard_normal((64,), dtype=np.float32) * np.float32(RELATION_SCALES["geo_emb/b"])
      w[scope + "/geo_conv/W"] = r_rng.standard_normal((1, 1, 64, 16), dtype=np.float32) * np.float32(RELATION_SCALES["geo_conv/W"])
      w[scope + "/geo_conv/b"] = r_rng.standard_normal((16,), dtype=np.float32) * np.float32(RELATION_SCALES["geo_conv/b"])
      for v in ("query_linear/W", "key_linear/W"):
        w[scope + "/" + v] = r_rng.standard_normal((dim, dim), dtype=np.float32) * np.float32(RELATION_SCALES[v] / np.sqrt(dim))
      w[scope + "/output_linear/W"] = r_rng.standard_normal((16 * dim, dim), dtype=np.float32) * np.float32(
          RELATION_SCALES["output_linear/W"] / np.sqrt(16.0 * dim))
  if getattr(config, "use_att_frcnn_head", False):
    # --use_att_frcnn_head (models.py:1064-1089) from a generator of its own.  attention/{W,b}: He-init and N(0, 0.02); any
    # finite values give the same graph.  att_trans reads the SUM of a RoI's 49 positions, which on the synthetic frames is close
    # to 49 times a single one (the FPN features of a RoI share a mean): He-init divided by 49, so that the branch is of the size
    # of the hidden vector it is added to (|att_trans| / |fc7| ~ 0.9 on the tests' frames)
    a_rng = np.random.default_rng([seed, 11])
    w["fastrcnn/attention/W"] = a_rng.standard_normal((3, 3, ch, 1), dtype=np.float32) * np.float32(np.sqrt(2.0 / (9 * ch)))
    w["fastrcnn/attention/b"] = a_rng.standard_normal((1,), dtype=np.float32) * np.float32(0.02)
    w["fastrcnn/att_trans/W"] = a_rng.standard_normal((ch, dim), dtype=np.float32) * np.float32(np.sqrt(2.0 / ch) / 49.0)
    w["fastrcnn/att_trans/b"] = a_rng.standard_normal((dim,), dtype=np.float32) * np.float32(0.02)
  return w


def synthetic_frames(batch, height, width, seed=1234):
  """Seeded synthetic BGR frames, uint8 [B,H,W,3]:
  smooth low-frequency background around 110 plus 40 solid noisy rectangles so
  that RPN / NMS see clustered, overlapping candidates."""
  rng = np.random.default_rng(seed)
  out = np.empty((batch, height, width, 3), np.uint8)
  for b in range(batch):
    gh, gw = height // 64 + 2, width // 64 + 2
    coarse = rng.normal(110.0, 20.0, (gh, gw, 3))
    ys = np.linspace(0, gh - 1.001, height)
    xs = np.linspace(0, gw - 1.001, width)
    y0 = np.floor(ys).astype(int); x0 = np.floor(xs).astype(int)
    fy = (ys - y0)[:, None, None]; fx = (xs - x0)[None, :, None]
    img = (coarse[y0][:, x0] * (1 - fy) * (1 - fx) +
           coarse[y0][:, x0 + 1] * (1 - fy) * fx +
           coarse[y0 + 1][:, x0] * fy * (1 - fx) +
           coarse[y0 + 1][:, x0 + 1] * fy * fx)
    img += rng.normal(0.0, 4.0, img.shape)
    for _ in range(40):
      rw = int(rng.uniform(16, min(400, width // 2)))
      rh = int(rng.uniform(16, min(400, height // 2)))
      x = int(rng.uniform(0, width - rw)); y = int(rng.uniform(0, height - rh))
      col = rng.uniform(0, 255, 3)
      img[y:y + rh, x:x + rw] = col + rng.normal(0, 6.0, (rh, rw, 3))
    out[b] = np.clip(np.rint(img), 0, 255).astype(np.uint8)
  return out


def select_partial_classes(weights, class_ids, num_class):
  """``--use_partial_classes`` (reference models.py:807-829, multi :2267-2287): the graph gathers
  label logits ``[0] + ids`` and box logits ``ids - 1`` (after the BG box was dropped).  Both are
  columns of a linear layer, so gathering the columns of ``fastrcnn/outputs/{class,box}`` once at
  load time yields the identical dot products; the head then runs with ``len(ids) + 1`` classes.
  Returns a new dict (the input is not modified)."""
  cols = np.asarray([0] + [int(i) for i in class_ids], np.int64)
  if cols.min() < 0 or cols.max() >= num_class:
    raise ValueError("partial class id outside [0, %d)" % num_class)
  out = dict(weights)
  W = np.asarray(weights["fastrcnn/outputs/class/W"]); b = np.asarray(weights["fastrcnn/outputs/class/b"])
  out["fastrcnn/outputs/class/W"] = np.ascontiguousarray(W[:, cols])
  out["fastrcnn/outputs/class/b"] = np.ascontiguousarray(b[cols])
  W = np.asarray(weights["fastrcnn/outputs/box/W"]); b = np.asarray(weights["fastrcnn/outputs/box/b"])
  W = W.reshape(W.shape[0], num_class, 4)[:, cols, :]
  out["fastrcnn/outputs/box/W"] = np.ascontiguousarray(W.reshape(W.shape[0], -1))
  out["fastrcnn/outputs/box/b"] = np.ascontiguousarray(b.reshape(num_class, 4)[cols].reshape(-1))
  return out


def expand_class_agnostic_box(weights, num_class):
  """``use_frcnn_class_agnostic`` (model versions 4-6; reference models.py:1126-1170 and
  :798-802): the head regresses ONE box per RoI (``fastrcnn/outputs/box`` is [dim, 4]) and the
  graph tiles it over the ``num_class - 1`` foreground classes.  Tiling the four weight columns
  over the classes once at load time yields the identical dot products for every class slot, so
  the per-class plan runs unchanged.  Returns a new dict."""
  W = np.asarray(weights["fastrcnn/outputs/box/W"]); b = np.asarray(weights["fastrcnn/outputs/box/b"])
  if W.shape[1] != 4 or b.shape[0] != 4:
    raise ValueError("class-agnostic box head expects fastrcnn/outputs/box/W of [dim, 4], got %s"
                     % (W.shape,))
  out = dict(weights)
  out["fastrcnn/outputs/box/W"] = np.ascontiguousarray(np.tile(W, (1, num_class)))
  out["fastrcnn/outputs/box/b"] = np.ascontiguousarray(np.tile(b, num_class))
  return out
