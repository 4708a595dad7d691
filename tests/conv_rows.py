"""The conv kernel ledger: for every row of the kernel table (the X(...) row list of csrc/odt_common.hpp) that a selection can
reach, the knobs and the small shapes under which the stand-alone conv ops run exactly that row -- and the helpers
tests/test_conv_rows.py and tests/test_ops.py use to prove it (ops.last_conv: what was launched; ops.conv_choice: what the
selection reports for the same shape).

Shapes.  Not model shapes: the smallest at which the tile logic can still be wrong.  Two images whose boundary lies inside
a tile, M = B Ho Wo a little over one or two tile heights and no multiple of it (the last tile is partial), odd Ho and Wo
(the nearest-2x residual"s coarse level is ceil(n / 2)), two or more n-tiles where the row"s n-tile allows, reductions of
two to nine stages:
  64-row tiles   2 x 5 x 7   (M = 70)       128-row tiles  2 x 9 x 9   (M = 162)
  256-row tiles  2 x 11 x 13 (M = 286)      512-row tiles  2 x 17 x 17 (M = 578)
  kw-reuse rows (Ho Wo >= 256): 2 x 17 x 17 (M = 578, the boundary inside tile 1), 512 x 64: 2 x 23 x 23 (Ho Wo >= 512, M = 1058)
  double-stage rows (H2D): K = 128 (the peeled steps only), 192, 320 (steady state)
  split-K: reductions whose stages do not divide by the factor -- the ranges [n k / s, n (k + 1) / s) have unequal lengths
  (10 or 18 sixteen-channel stages / 5 or 9 thirty-two-channel ones in four ranges; 33 and 45 stages, 9 (slice, kh) groups in two)

Features of an entry: "relu" (bias + ReLU; every entry has a bias), "res1" (same-shape residual), "res2" (nearest-2x
residual, odd Ho, Wo), "off" (output offset (1, 1) into a zeroed buffer), "s2" (stride 2), "d2" (dilation 2), "cat1" / "cat2"
(ops.conv2d_cat: a second K-concatenated source of 32 / 96 channels at stride 1 / 2).
"""
import os

import numpy as np

from common import torch_conv_nhwc
from object_detection_tracking_amd import ops

F = np.float32
FEATURES = ("relu", "res1", "res2", "off", "s2", "d2", "cat1", "cat2")
CAT = {"cat1": (32, 1), "cat2": (96, 2)}      # second source: channels, stride


def _env(**kw):
  e = {"ODT_CONV_SPLIT": "1", "ODT_CONV_SPLIT_MINTILES": "1", "ODT_CONV_SPLIT3_MINTILES": "1"}
  e.update(("ODT_CONV_" + k, str(v)) for k, v in kw.items())
  return e


def _f32(tile, stages, fine):
  return {"ODT_CONV_SPLIT": "0", "ODT_CONV_TILE": str(tile), "ODT_CONV_STAGES": str(stages), "ODT_CONV_FINE": str(fine)}


# the knob sets (every inherited ODT_* variable is removed first: use_env)
PIPE1 = _env(SPLIT_PIPE=1)
S3_256 = _env(SPLIT_PIPE=3, SPLIT3_BM=256)      # (Ho Wo < 256: the kw-reuse kernel does not take the layer; >= 256: it does)
S3_128 = _env(SPLIT_PIPE=3, SPLIT3_BM=128)
S3_256_K4 = _env(SPLIT_PIPE=3, SPLIT3_BM=256, SPLIT3_FORCE_SPLITK=4)
S3_128_K4 = _env(SPLIT_PIPE=3, SPLIT3_BM=128, SPLIT3_FORCE_SPLITK=4)
H2_256 = _env(SPLIT_PIPE=2, SPLIT3_BM=256)
H2_256_K4 = _env(SPLIT_PIPE=2, SPLIT3_BM=256, SPLIT3_FORCE_SPLITK=4)
H2_128 = _env(SPLIT_PIPE=2, SPLIT3_BM=128)
H2_128_K4 = _env(SPLIT_PIPE=2, SPLIT3_BM=128, SPLIT3_FORCE_SPLITK=4)
# 64-row tiles: M = 70 and Cout = 256 give 2 tiles of 128 x 128 and 4 of 64 x 128 -- 2 < MINTILES = 3 <= 4 (rule_h2_64_rows)
H2_64x128 = _env(SPLIT_PIPE=2, SPLIT3_BM=128, SPLIT3_MINTILES=3, H2_BM64=1, H2_BK64=0)
H2_64x64 = _env(SPLIT_PIPE=2, SPLIT3_BM=128, SPLIT3_MINTILES=3, H2_BM64=3, H2_BK64=0)
H2D_64x128 = _env(SPLIT_PIPE=2, SPLIT3_BM=128, SPLIT3_MINTILES=3, H2_BM64=1)
H2D_64x64 = _env(SPLIT_PIPE=2, SPLIT3_BM=128, SPLIT3_MINTILES=3, H2_BM64=3)
H2_64_K2 = _env(SPLIT_PIPE=2, SPLIT3_BM=128, SPLIT3_MINTILES=3, H2_BM64=2)      # K > 1024: the reduction cut in two
H2_N64 = _env(SPLIT_PIPE=2, H2_N64_BM512=0)
H2_N64_512 = _env(SPLIT_PIPE=2, H2_N64_BM512=2, SPLIT3_KWR=0)      # (KWR=0: the 3x3 entries would take H2K_256x64)
H2K_512 = _env(SPLIT_PIPE=2, SPLIT3_BM=256, H2_N64_BM512=2)
H2K_FEW = _env(SPLIT_PIPE=2, SPLIT3_MINTILES=8)      # rule_h2k_few_rows: 6 tiles of 256 x 128 < 8 -> two ranges
F32_T1S1F0 = _f32(1, 1, 0)
F32_T1S1F1 = _f32(1, 1, 1)
F32_T1S2F0 = _f32(1, 2, 0)
F32_T1S2F1 = _f32(1, 2, 1)
F32_T2S1F0 = _f32(2, 1, 0)
F32_T2S1F1 = _f32(2, 1, 1)
F32_T2S2F0 = _f32(2, 2, 0)
F32_T2S2F1 = _f32(2, 2, 1)
F32_T3S1F0 = _f32(3, 1, 0)
F32_T3S1F1 = _f32(3, 1, 1)
F32_T3S2F0 = _f32(3, 2, 0)
F32_T3S2F1 = _f32(3, 2, 1)

LEDGER = [
    # row, split-K, env, case (B, H, W, Cin, Cout, k, stride, dil, pad_t, pad_l, Ho, Wo, relu -- test_ops.CONV_CASES" layout;
    # for "cat1" / "cat2": the first source), features
    # F32_128x64_S1
    ("F32_128x64_S1",       0, F32_T1S1F0,  (2, 17, 17, 96, 72, 1, 2, 1, 0, 0, 9, 9, True),            ("relu", "res1", "s2")),
    ("F32_128x64_S1",       0, F32_T1S1F0,  (2, 9, 9, 32, 40, 3, 1, 2, 2, 2, 9, 9, False),             ("d2", "res2")),
    ("F32_128x64_S1",       0, F32_T1S1F0,  (2, 9, 9, 32, 40, 3, 1, 1, 1, 1, 9, 9, True),              ("relu", "off")),
    ("F32_128x64_S1",       0, F32_T1S1F0,  (2, 9, 9, 64, 40, 1, 1, 1, 0, 0, 9, 9, False),             ("cat1",)),
    ("F32_128x64_S1",       0, F32_T1S1F0,  (2, 9, 9, 64, 72, 1, 1, 1, 0, 0, 9, 9, True),              ("relu", "cat2")),
    # F32_128x64_S1_FINE
    ("F32_128x64_S1_FINE",  0, F32_T1S1F1,  (2, 17, 17, 96, 72, 1, 2, 1, 0, 0, 9, 9, True),            ("relu", "res1", "s2")),
    ("F32_128x64_S1_FINE",  0, F32_T1S1F1,  (2, 9, 9, 32, 40, 3, 1, 2, 2, 2, 9, 9, False),             ("d2", "res2")),
    ("F32_128x64_S1_FINE",  0, F32_T1S1F1,  (2, 9, 9, 32, 40, 3, 1, 1, 1, 1, 9, 9, True),              ("relu", "off")),
    ("F32_128x64_S1_FINE",  0, F32_T1S1F1,  (2, 9, 9, 64, 40, 1, 1, 1, 0, 0, 9, 9, False),             ("cat1",)),
    ("F32_128x64_S1_FINE",  0, F32_T1S1F1,  (2, 9, 9, 64, 72, 1, 1, 1, 0, 0, 9, 9, True),              ("relu", "cat2")),
    # F32_128x64_S2
    ("F32_128x64_S2",       0, F32_T1S2F0,  (2, 17, 17, 96, 72, 1, 2, 1, 0, 0, 9, 9, True),            ("relu", "res1", "s2")),
    ("F32_128x64_S2",       0, F32_T1S2F0,  (2, 9, 9, 32, 40, 3, 1, 2, 2, 2, 9, 9, False),             ("d2", "res2")),
    ("F32_128x64_S2",       0, F32_T1S2F0,  (2, 9, 9, 32, 40, 3, 1, 1, 1, 1, 9, 9, True),              ("relu", "off")),
    ("F32_128x64_S2",       0, F32_T1S2F0,  (2, 9, 9, 64, 40, 1, 1, 1, 0, 0, 9, 9, False),             ("cat1",)),
    ("F32_128x64_S2",       0, F32_T1S2F0,  (2, 9, 9, 64, 72, 1, 1, 1, 0, 0, 9, 9, True),              ("relu", "cat2")),
    # F32_128x64_S2_FINE
    ("F32_128x64_S2_FINE",  0, F32_T1S2F1,  (2, 17, 17, 96, 72, 1, 2, 1, 0, 0, 9, 9, True),            ("relu", "res1", "s2")),
    ("F32_128x64_S2_FINE",  0, F32_T1S2F1,  (2, 9, 9, 32, 40, 3, 1, 2, 2, 2, 9, 9, False),             ("d2", "res2")),
    ("F32_128x64_S2_FINE",  0, F32_T1S2F1,  (2, 9, 9, 32, 40, 3, 1, 1, 1, 1, 9, 9, True),              ("relu", "off")),
    ("F32_128x64_S2_FINE",  0, F32_T1S2F1,  (2, 9, 9, 64, 40, 1, 1, 1, 0, 0, 9, 9, False),             ("cat1",)),
    ("F32_128x64_S2_FINE",  0, F32_T1S2F1,  (2, 9, 9, 64, 72, 1, 1, 1, 0, 0, 9, 9, True),              ("relu", "cat2")),
    # F32_64x64_S1
    ("F32_64x64_S1",        0, F32_T2S1F0,  (2, 9, 13, 96, 72, 1, 2, 1, 0, 0, 5, 7, True),             ("relu", "res1", "s2")),
    ("F32_64x64_S1",        0, F32_T2S1F0,  (2, 5, 7, 32, 40, 3, 1, 2, 2, 2, 5, 7, False),             ("d2", "res2")),
    ("F32_64x64_S1",        0, F32_T2S1F0,  (2, 5, 7, 32, 40, 3, 1, 1, 1, 1, 5, 7, True),              ("relu", "off")),
    ("F32_64x64_S1",        0, F32_T2S1F0,  (2, 5, 7, 64, 40, 1, 1, 1, 0, 0, 5, 7, False),             ("cat1",)),
    ("F32_64x64_S1",        0, F32_T2S1F0,  (2, 5, 7, 64, 72, 1, 1, 1, 0, 0, 5, 7, True),              ("relu", "cat2")),
    # F32_64x64_S1_FINE
    ("F32_64x64_S1_FINE",   0, F32_T2S1F1,  (2, 9, 13, 96, 72, 1, 2, 1, 0, 0, 5, 7, True),             ("relu", "res1", "s2")),
    ("F32_64x64_S1_FINE",   0, F32_T2S1F1,  (2, 5, 7, 32, 40, 3, 1, 2, 2, 2, 5, 7, False),             ("d2", "res2")),
    ("F32_64x64_S1_FINE",   0, F32_T2S1F1,  (2, 5, 7, 32, 40, 3, 1, 1, 1, 1, 5, 7, True),              ("relu", "off")),
    ("F32_64x64_S1_FINE",   0, F32_T2S1F1,  (2, 5, 7, 64, 40, 1, 1, 1, 0, 0, 5, 7, False),             ("cat1",)),
    ("F32_64x64_S1_FINE",   0, F32_T2S1F1,  (2, 5, 7, 64, 72, 1, 1, 1, 0, 0, 5, 7, True),              ("relu", "cat2")),
    # F32_64x64_S2
    ("F32_64x64_S2",        0, F32_T2S2F0,  (2, 9, 13, 96, 72, 1, 2, 1, 0, 0, 5, 7, True),             ("relu", "res1", "s2")),
    ("F32_64x64_S2",        0, F32_T2S2F0,  (2, 5, 7, 32, 40, 3, 1, 2, 2, 2, 5, 7, False),             ("d2", "res2")),
    ("F32_64x64_S2",        0, F32_T2S2F0,  (2, 5, 7, 32, 40, 3, 1, 1, 1, 1, 5, 7, True),              ("relu", "off")),
    ("F32_64x64_S2",        0, F32_T2S2F0,  (2, 5, 7, 64, 40, 1, 1, 1, 0, 0, 5, 7, False),             ("cat1",)),
    ("F32_64x64_S2",        0, F32_T2S2F0,  (2, 5, 7, 64, 72, 1, 1, 1, 0, 0, 5, 7, True),              ("relu", "cat2")),
    # F32_64x64_S2_FINE
    ("F32_64x64_S2_FINE",   0, F32_T2S2F1,  (2, 9, 13, 96, 72, 1, 2, 1, 0, 0, 5, 7, True),             ("relu", "res1", "s2")),
    ("F32_64x64_S2_FINE",   0, F32_T2S2F1,  (2, 5, 7, 32, 40, 3, 1, 2, 2, 2, 5, 7, False),             ("d2", "res2")),
    ("F32_64x64_S2_FINE",   0, F32_T2S2F1,  (2, 5, 7, 32, 40, 3, 1, 1, 1, 1, 5, 7, True),              ("relu", "off")),
    ("F32_64x64_S2_FINE",   0, F32_T2S2F1,  (2, 5, 7, 64, 40, 1, 1, 1, 0, 0, 5, 7, False),             ("cat1",)),
    ("F32_64x64_S2_FINE",   0, F32_T2S2F1,  (2, 5, 7, 64, 72, 1, 1, 1, 0, 0, 5, 7, True),              ("relu", "cat2")),
    # F32_128x128_S1
    ("F32_128x128_S1",      0, F32_T3S1F0,  (2, 17, 17, 96, 136, 1, 2, 1, 0, 0, 9, 9, True),           ("relu", "res1", "s2")),
    ("F32_128x128_S1",      0, F32_T3S1F0,  (2, 9, 9, 32, 72, 3, 1, 2, 2, 2, 9, 9, False),             ("d2", "res2")),
    ("F32_128x128_S1",      0, F32_T3S1F0,  (2, 9, 9, 32, 72, 3, 1, 1, 1, 1, 9, 9, True),              ("relu", "off")),
    ("F32_128x128_S1",      0, F32_T3S1F0,  (2, 9, 9, 64, 72, 1, 1, 1, 0, 0, 9, 9, False),             ("cat1",)),
    ("F32_128x128_S1",      0, F32_T3S1F0,  (2, 9, 9, 64, 136, 1, 1, 1, 0, 0, 9, 9, True),             ("relu", "cat2")),
    # F32_128x128_S1_FINE
    ("F32_128x128_S1_FINE", 0, F32_T3S1F1,  (2, 17, 17, 96, 136, 1, 2, 1, 0, 0, 9, 9, True),           ("relu", "res1", "s2")),
    ("F32_128x128_S1_FINE", 0, F32_T3S1F1,  (2, 9, 9, 32, 72, 3, 1, 2, 2, 2, 9, 9, False),             ("d2", "res2")),
    ("F32_128x128_S1_FINE", 0, F32_T3S1F1,  (2, 9, 9, 32, 72, 3, 1, 1, 1, 1, 9, 9, True),              ("relu", "off")),
    ("F32_128x128_S1_FINE", 0, F32_T3S1F1,  (2, 9, 9, 64, 72, 1, 1, 1, 0, 0, 9, 9, False),             ("cat1",)),
    ("F32_128x128_S1_FINE", 0, F32_T3S1F1,  (2, 9, 9, 64, 136, 1, 1, 1, 0, 0, 9, 9, True),             ("relu", "cat2")),
    # F32_128x128_S2
    ("F32_128x128_S2",      0, F32_T3S2F0,  (2, 17, 17, 96, 136, 1, 2, 1, 0, 0, 9, 9, True),           ("relu", "res1", "s2")),
    ("F32_128x128_S2",      0, F32_T3S2F0,  (2, 9, 9, 32, 72, 3, 1, 2, 2, 2, 9, 9, False),             ("d2", "res2")),
    ("F32_128x128_S2",      0, F32_T3S2F0,  (2, 9, 9, 32, 72, 3, 1, 1, 1, 1, 9, 9, True),              ("relu", "off")),
    ("F32_128x128_S2",      0, F32_T3S2F0,  (2, 9, 9, 64, 72, 1, 1, 1, 0, 0, 9, 9, False),             ("cat1",)),
    ("F32_128x128_S2",      0, F32_T3S2F0,  (2, 9, 9, 64, 136, 1, 1, 1, 0, 0, 9, 9, True),             ("relu", "cat2")),
    # F32_128x128_S2_FINE
    ("F32_128x128_S2_FINE", 0, F32_T3S2F1,  (2, 17, 17, 96, 136, 1, 2, 1, 0, 0, 9, 9, True),           ("relu", "res1", "s2")),
    ("F32_128x128_S2_FINE", 0, F32_T3S2F1,  (2, 9, 9, 32, 72, 3, 1, 2, 2, 2, 9, 9, False),             ("d2", "res2")),
    ("F32_128x128_S2_FINE", 0, F32_T3S2F1,  (2, 9, 9, 32, 72, 3, 1, 1, 1, 1, 9, 9, True),              ("relu", "off")),
    ("F32_128x128_S2_FINE", 0, F32_T3S2F1,  (2, 9, 9, 64, 72, 1, 1, 1, 0, 0, 9, 9, False),             ("cat1",)),
    ("F32_128x128_S2_FINE", 0, F32_T3S2F1,  (2, 9, 9, 64, 136, 1, 1, 1, 0, 0, 9, 9, True),             ("relu", "cat2")),
    # SPLIT1_128x256
    ("SPLIT1_128x256",      1, PIPE1,       (2, 17, 17, 96, 512, 1, 2, 1, 0, 0, 9, 9, True),           ("relu", "res1", "s2")),
    ("SPLIT1_128x256",      1, PIPE1,       (2, 9, 9, 32, 256, 3, 1, 2, 2, 2, 9, 9, False),            ("d2", "res2")),
    ("SPLIT1_128x256",      1, PIPE1,       (2, 9, 9, 32, 256, 3, 1, 1, 1, 1, 9, 9, True),             ("relu", "off")),
    ("SPLIT1_128x256",      1, PIPE1,       (2, 9, 9, 64, 256, 1, 1, 1, 0, 0, 9, 9, False),            ("cat1",)),
    ("SPLIT1_128x256",      1, PIPE1,       (2, 9, 9, 64, 512, 1, 1, 1, 0, 0, 9, 9, True),             ("relu", "cat2")),
    # SPLIT1_256x128
    ("SPLIT1_256x128",      1, PIPE1,       (2, 21, 25, 96, 384, 1, 2, 1, 0, 0, 11, 13, True),         ("relu", "res1", "s2")),
    ("SPLIT1_256x128",      1, PIPE1,       (2, 11, 13, 32, 128, 3, 1, 2, 2, 2, 11, 13, False),        ("d2", "res2")),
    ("SPLIT1_256x128",      1, PIPE1,       (2, 11, 13, 32, 128, 3, 1, 1, 1, 1, 11, 13, True),         ("relu", "off")),
    ("SPLIT1_256x128",      1, PIPE1,       (2, 11, 13, 64, 128, 1, 1, 1, 0, 0, 11, 13, False),        ("cat1",)),
    ("SPLIT1_256x128",      1, PIPE1,       (2, 11, 13, 64, 384, 1, 1, 1, 0, 0, 11, 13, True),         ("relu", "cat2")),
    # SPLIT1_256x64
    ("SPLIT1_256x64",       1, PIPE1,       (2, 21, 25, 96, 192, 1, 2, 1, 0, 0, 11, 13, True),         ("relu", "res1", "s2")),
    ("SPLIT1_256x64",       1, PIPE1,       (2, 11, 13, 32, 64, 3, 1, 2, 2, 2, 11, 13, False),         ("d2", "res2")),
    ("SPLIT1_256x64",       1, PIPE1,       (2, 11, 13, 32, 64, 3, 1, 1, 1, 1, 11, 13, True),          ("relu", "off")),
    ("SPLIT1_256x64",       1, PIPE1,       (2, 11, 13, 64, 64, 1, 1, 1, 0, 0, 11, 13, False),         ("cat1",)),
    ("SPLIT1_256x64",       1, PIPE1,       (2, 11, 13, 64, 192, 1, 1, 1, 0, 0, 11, 13, True),         ("relu", "cat2")),
    # SPLIT3_256x256
    ("SPLIT3_256x256",      1, S3_256,      (2, 21, 25, 96, 512, 1, 2, 1, 0, 0, 11, 13, True),         ("relu", "res1", "s2")),
    ("SPLIT3_256x256",      1, S3_256,      (2, 11, 13, 32, 256, 3, 1, 2, 2, 2, 11, 13, False),        ("d2", "res2")),
    ("SPLIT3_256x256",      1, S3_256,      (2, 11, 13, 32, 256, 3, 1, 1, 1, 1, 11, 13, True),         ("relu", "off")),
    ("SPLIT3_256x256",      1, S3_256,      (2, 11, 13, 64, 256, 1, 1, 1, 0, 0, 11, 13, False),        ("cat1",)),
    ("SPLIT3_256x256",      1, S3_256,      (2, 11, 13, 64, 512, 1, 1, 1, 0, 0, 11, 13, True),         ("relu", "cat2")),
    # SPLIT3_256x256, split-K
    ("SPLIT3_256x256",      4, S3_256_K4,   (2, 21, 25, 160, 512, 1, 2, 1, 0, 0, 11, 13, True),        ("relu", "res1", "s2")),
    ("SPLIT3_256x256",      4, S3_256_K4,   (2, 11, 13, 32, 256, 3, 1, 2, 2, 2, 11, 13, False),        ("d2", "res2")),
    ("SPLIT3_256x256",      4, S3_256_K4,   (2, 11, 13, 32, 256, 3, 1, 1, 1, 1, 11, 13, True),         ("relu", "off")),
    # SPLIT3_256x128
    ("SPLIT3_256x128",      1, S3_256,      (2, 21, 25, 96, 384, 1, 2, 1, 0, 0, 11, 13, True),         ("relu", "res1", "s2")),
    ("SPLIT3_256x128",      1, S3_256,      (2, 11, 13, 32, 128, 3, 1, 2, 2, 2, 11, 13, False),        ("d2", "res2")),
    ("SPLIT3_256x128",      1, S3_256,      (2, 11, 13, 32, 128, 3, 1, 1, 1, 1, 11, 13, True),         ("relu", "off")),
    ("SPLIT3_256x128",      1, S3_256,      (2, 11, 13, 64, 128, 1, 1, 1, 0, 0, 11, 13, False),        ("cat1",)),
    ("SPLIT3_256x128",      1, S3_256,      (2, 11, 13, 64, 384, 1, 1, 1, 0, 0, 11, 13, True),         ("relu", "cat2")),
    # SPLIT3_256x128, split-K
    ("SPLIT3_256x128",      4, S3_256_K4,   (2, 21, 25, 160, 384, 1, 2, 1, 0, 0, 11, 13, True),        ("relu", "res1", "s2")),
    ("SPLIT3_256x128",      4, S3_256_K4,   (2, 11, 13, 32, 128, 3, 1, 2, 2, 2, 11, 13, False),        ("d2", "res2")),
    ("SPLIT3_256x128",      4, S3_256_K4,   (2, 11, 13, 32, 128, 3, 1, 1, 1, 1, 11, 13, True),         ("relu", "off")),
    # SPLIT3_256x64
    ("SPLIT3_256x64",       1, S3_256,      (2, 21, 25, 96, 192, 1, 2, 1, 0, 0, 11, 13, True),         ("relu", "res1", "s2")),
    ("SPLIT3_256x64",       1, S3_256,      (2, 11, 13, 32, 64, 3, 1, 2, 2, 2, 11, 13, False),         ("d2", "res2")),
    ("SPLIT3_256x64",       1, S3_256,      (2, 11, 13, 32, 64, 3, 1, 1, 1, 1, 11, 13, True),          ("relu", "off")),
    ("SPLIT3_256x64",       1, S3_256,      (2, 11, 13, 64, 64, 1, 1, 1, 0, 0, 11, 13, False),         ("cat1",)),
    ("SPLIT3_256x64",       1, S3_256,      (2, 11, 13, 64, 192, 1, 1, 1, 0, 0, 11, 13, True),         ("relu", "cat2")),
    # SPLIT3_256x64, split-K
    ("SPLIT3_256x64",       4, S3_256_K4,   (2, 21, 25, 160, 192, 1, 2, 1, 0, 0, 11, 13, True),        ("relu", "res1", "s2")),
    ("SPLIT3_256x64",       4, S3_256_K4,   (2, 11, 13, 32, 64, 3, 1, 2, 2, 2, 11, 13, False),         ("d2", "res2")),
    ("SPLIT3_256x64",       4, S3_256_K4,   (2, 11, 13, 32, 64, 3, 1, 1, 1, 1, 11, 13, True),          ("relu", "off")),
    # SPLIT3_128x256
    ("SPLIT3_128x256",      1, S3_128,      (2, 17, 17, 96, 512, 1, 2, 1, 0, 0, 9, 9, True),           ("relu", "res1", "s2")),
    ("SPLIT3_128x256",      1, S3_128,      (2, 9, 9, 32, 256, 3, 1, 2, 2, 2, 9, 9, False),            ("d2", "res2")),
    ("SPLIT3_128x256",      1, S3_128,      (2, 9, 9, 32, 256, 3, 1, 1, 1, 1, 9, 9, True),             ("relu", "off")),
    ("SPLIT3_128x256",      1, S3_128,      (2, 9, 9, 64, 256, 1, 1, 1, 0, 0, 9, 9, False),            ("cat1",)),
    ("SPLIT3_128x256",      1, S3_128,      (2, 9, 9, 64, 512, 1, 1, 1, 0, 0, 9, 9, True),             ("relu", "cat2")),
    # SPLIT3_128x256, split-K
    ("SPLIT3_128x256",      4, S3_128_K4,   (2, 17, 17, 160, 512, 1, 2, 1, 0, 0, 9, 9, True),          ("relu", "res1", "s2")),
    ("SPLIT3_128x256",      4, S3_128_K4,   (2, 9, 9, 32, 256, 3, 1, 2, 2, 2, 9, 9, False),            ("d2", "res2")),
    ("SPLIT3_128x256",      4, S3_128_K4,   (2, 9, 9, 32, 256, 3, 1, 1, 1, 1, 9, 9, True),             ("relu", "off")),
    # SPLIT3_128x128
    ("SPLIT3_128x128",      1, S3_128,      (2, 17, 17, 96, 384, 1, 2, 1, 0, 0, 9, 9, True),           ("relu", "res1", "s2")),
    ("SPLIT3_128x128",      1, S3_128,      (2, 9, 9, 32, 128, 3, 1, 2, 2, 2, 9, 9, False),            ("d2", "res2")),
    ("SPLIT3_128x128",      1, S3_128,      (2, 9, 9, 32, 128, 3, 1, 1, 1, 1, 9, 9, True),             ("relu", "off")),
    ("SPLIT3_128x128",      1, S3_128,      (2, 9, 9, 64, 128, 1, 1, 1, 0, 0, 9, 9, False),            ("cat1",)),
    ("SPLIT3_128x128",      1, S3_128,      (2, 9, 9, 64, 384, 1, 1, 1, 0, 0, 9, 9, True),             ("relu", "cat2")),
    # SPLIT3_128x128, split-K
    ("SPLIT3_128x128",      4, S3_128_K4,   (2, 17, 17, 160, 384, 1, 2, 1, 0, 0, 9, 9, True),          ("relu", "res1", "s2")),
    ("SPLIT3_128x128",      4, S3_128_K4,   (2, 9, 9, 32, 128, 3, 1, 2, 2, 2, 9, 9, False),            ("d2", "res2")),
    ("SPLIT3_128x128",      4, S3_128_K4,   (2, 9, 9, 32, 128, 3, 1, 1, 1, 1, 9, 9, True),             ("relu", "off")),
    # SPLIT3K_256x256
    ("SPLIT3K_256x256",     1, S3_256,      (2, 17, 17, 32, 256, 3, 1, 2, 2, 2, 17, 17, False),        ("d2", "res2")),
    ("SPLIT3K_256x256",     1, S3_256,      (2, 17, 17, 32, 512, 3, 1, 1, 1, 1, 17, 17, True),         ("relu", "res1")),
    ("SPLIT3K_256x256",     1, S3_256,      (2, 17, 17, 32, 256, 3, 1, 1, 1, 1, 17, 17, True),         ("relu", "off")),
    # SPLIT3K_256x128
    ("SPLIT3K_256x128",     1, S3_256,      (2, 17, 17, 32, 128, 3, 1, 2, 2, 2, 17, 17, False),        ("d2", "res2")),
    ("SPLIT3K_256x128",     1, S3_256,      (2, 17, 17, 32, 384, 3, 1, 1, 1, 1, 17, 17, True),         ("relu", "res1")),
    ("SPLIT3K_256x128",     1, S3_256,      (2, 17, 17, 32, 128, 3, 1, 1, 1, 1, 17, 17, True),         ("relu", "off")),
    # SPLIT3K_256x64
    ("SPLIT3K_256x64",      1, S3_256,      (2, 17, 17, 32, 64, 3, 1, 2, 2, 2, 17, 17, False),         ("d2", "res2")),
    ("SPLIT3K_256x64",      1, S3_256,      (2, 17, 17, 32, 192, 3, 1, 1, 1, 1, 17, 17, True),         ("relu", "res1")),
    ("SPLIT3K_256x64",      1, S3_256,      (2, 17, 17, 32, 64, 3, 1, 1, 1, 1, 17, 17, True),          ("relu", "off")),
    # H2_64x64
    ("H2_64x64",            1, H2_64x64,    (2, 9, 13, 96, 256, 1, 2, 1, 0, 0, 5, 7, True),            ("relu", "res1", "s2")),
    ("H2_64x64",            1, H2_64x64,    (2, 5, 7, 32, 256, 3, 1, 2, 2, 2, 5, 7, False),            ("d2", "res2")),
    ("H2_64x64",            1, H2_64x64,    (2, 5, 7, 32, 256, 3, 1, 1, 1, 1, 5, 7, True),             ("relu", "off")),
    ("H2_64x64",            1, H2_64x64,    (2, 5, 7, 64, 256, 1, 1, 1, 0, 0, 5, 7, False),            ("cat1",)),
    ("H2_64x64",            1, H2_64x64,    (2, 5, 7, 64, 256, 1, 1, 1, 0, 0, 5, 7, True),             ("relu", "cat2")),
    # H2_64x128
    ("H2_64x128",           1, H2_64x128,   (2, 9, 13, 96, 256, 1, 2, 1, 0, 0, 5, 7, True),            ("relu", "res1", "s2")),
    ("H2_64x128",           1, H2_64x128,   (2, 5, 7, 32, 256, 3, 1, 2, 2, 2, 5, 7, False),            ("d2", "res2")),
    ("H2_64x128",           1, H2_64x128,   (2, 5, 7, 32, 256, 3, 1, 1, 1, 1, 5, 7, True),             ("relu", "off")),
    ("H2_64x128",           1, H2_64x128,   (2, 5, 7, 64, 256, 1, 1, 1, 0, 0, 5, 7, False),            ("cat1",)),
    ("H2_64x128",           1, H2_64x128,   (2, 5, 7, 64, 256, 1, 1, 1, 0, 0, 5, 7, True),             ("relu", "cat2")),
    # H2_64x128, split-K
    ("H2_64x128",           2, H2_64_K2,    (2, 9, 13, 1056, 256, 1, 2, 1, 0, 0, 5, 7, True),          ("relu", "res1", "s2")),
    ("H2_64x128",           2, H2_64_K2,    (2, 5, 7, 160, 256, 3, 1, 2, 2, 2, 5, 7, False),           ("d2", "res2")),
    ("H2_64x128",           2, H2_64_K2,    (2, 5, 7, 160, 256, 3, 1, 1, 1, 1, 5, 7, True),            ("relu", "off")),
    # H2_512x64
    ("H2_512x64",           1, H2_N64_512,  (2, 33, 33, 96, 64, 1, 2, 1, 0, 0, 17, 17, True),          ("relu", "res1", "s2")),
    ("H2_512x64",           1, H2_N64_512,  (2, 17, 17, 32, 64, 3, 1, 2, 2, 2, 17, 17, False),         ("d2", "res2")),
    ("H2_512x64",           1, H2_N64_512,  (2, 17, 17, 32, 64, 3, 1, 1, 1, 1, 17, 17, True),          ("relu", "off")),
    # H2_128x64
    ("H2_128x64",           1, H2_N64,      (2, 17, 17, 96, 192, 1, 2, 1, 0, 0, 9, 9, True),           ("relu", "res1", "s2")),
    ("H2_128x64",           1, H2_N64,      (2, 9, 9, 32, 64, 3, 1, 2, 2, 2, 9, 9, False),             ("d2", "res2")),
    ("H2_128x64",           1, H2_N64,      (2, 9, 9, 32, 64, 3, 1, 1, 1, 1, 9, 9, True),              ("relu", "off")),
    # H2_256x256
    ("H2_256x256",          1, H2_256,      (2, 21, 25, 96, 512, 1, 2, 1, 0, 0, 11, 13, True),         ("relu", "res1", "s2")),
    ("H2_256x256",          1, H2_256,      (2, 11, 13, 32, 256, 3, 1, 2, 2, 2, 11, 13, False),        ("d2", "res2")),
    ("H2_256x256",          1, H2_256,      (2, 11, 13, 32, 256, 3, 1, 1, 1, 1, 11, 13, True),         ("relu", "off")),
    ("H2_256x256",          1, H2_256,      (2, 11, 13, 64, 256, 1, 1, 1, 0, 0, 11, 13, False),        ("cat1",)),
    ("H2_256x256",          1, H2_256,      (2, 11, 13, 64, 512, 1, 1, 1, 0, 0, 11, 13, True),         ("relu", "cat2")),
    # H2_256x256, split-K
    ("H2_256x256",          4, H2_256_K4,   (2, 21, 25, 160, 512, 1, 2, 1, 0, 0, 11, 13, True),        ("relu", "res1", "s2")),
    ("H2_256x256",          4, H2_256_K4,   (2, 11, 13, 32, 256, 3, 1, 2, 2, 2, 11, 13, False),        ("d2", "res2")),
    ("H2_256x256",          4, H2_256_K4,   (2, 11, 13, 32, 256, 3, 1, 1, 1, 1, 11, 13, True),         ("relu", "off")),
    # H2_256x128
    ("H2_256x128",          1, H2_256,      (2, 21, 25, 96, 384, 1, 2, 1, 0, 0, 11, 13, True),         ("relu", "res1", "s2")),
    ("H2_256x128",          1, H2_256,      (2, 11, 13, 32, 128, 3, 1, 2, 2, 2, 11, 13, False),        ("d2", "res2")),
    ("H2_256x128",          1, H2_256,      (2, 11, 13, 32, 128, 3, 1, 1, 1, 1, 11, 13, True),         ("relu", "off")),
    ("H2_256x128",          1, H2_256,      (2, 11, 13, 64, 128, 1, 1, 1, 0, 0, 11, 13, False),        ("cat1",)),
    ("H2_256x128",          1, H2_256,      (2, 11, 13, 64, 384, 1, 1, 1, 0, 0, 11, 13, True),         ("relu", "cat2")),
    # H2_256x128, split-K
    ("H2_256x128",          4, H2_256_K4,   (2, 21, 25, 160, 384, 1, 2, 1, 0, 0, 11, 13, True),        ("relu", "res1", "s2")),
    ("H2_256x128",          4, H2_256_K4,   (2, 11, 13, 32, 128, 3, 1, 2, 2, 2, 11, 13, False),        ("d2", "res2")),
    ("H2_256x128",          4, H2_256_K4,   (2, 11, 13, 32, 128, 3, 1, 1, 1, 1, 11, 13, True),         ("relu", "off")),
    # H2_128x128
    ("H2_128x128",          1, H2_128,      (2, 17, 17, 96, 256, 1, 2, 1, 0, 0, 9, 9, True),           ("relu", "res1", "s2")),
    ("H2_128x128",          1, H2_128,      (2, 9, 9, 32, 256, 3, 1, 2, 2, 2, 9, 9, False),            ("d2", "res2")),
    ("H2_128x128",          1, H2_128,      (2, 9, 9, 32, 256, 3, 1, 1, 1, 1, 9, 9, True),             ("relu", "off")),
    ("H2_128x128",          1, H2_128,      (2, 9, 9, 64, 256, 1, 1, 1, 0, 0, 9, 9, False),            ("cat1",)),
    ("H2_128x128",          1, H2_128,      (2, 9, 9, 64, 256, 1, 1, 1, 0, 0, 9, 9, True),             ("relu", "cat2")),
    # H2_128x128, split-K
    ("H2_128x128",          4, H2_128_K4,   (2, 17, 17, 160, 256, 1, 2, 1, 0, 0, 9, 9, True),          ("relu", "res1", "s2")),
    ("H2_128x128",          4, H2_128_K4,   (2, 9, 9, 32, 256, 3, 1, 2, 2, 2, 9, 9, False),            ("d2", "res2")),
    ("H2_128x128",          4, H2_128_K4,   (2, 9, 9, 32, 256, 3, 1, 1, 1, 1, 9, 9, True),             ("relu", "off")),
    # H2D_64x64
    ("H2D_64x64",           1, H2D_64x64,   (2, 5, 7, 128, 256, 1, 1, 1, 0, 0, 5, 7, True),            ("relu",)),
    ("H2D_64x64",           1, H2D_64x64,   (2, 5, 7, 128, 256, 1, 1, 1, 0, 0, 5, 7, True),            ("relu", "off")),
    ("H2D_64x64",           1, H2D_64x64,   (2, 5, 7, 192, 256, 1, 1, 1, 0, 0, 5, 7, True),            ("relu", "res1")),
    ("H2D_64x64",           1, H2D_64x64,   (2, 5, 7, 320, 256, 1, 1, 1, 0, 0, 5, 7, False),           ("res2",)),
    # H2D_64x128
    ("H2D_64x128",          1, H2D_64x128,  (2, 5, 7, 128, 256, 1, 1, 1, 0, 0, 5, 7, True),            ("relu",)),
    ("H2D_64x128",          1, H2D_64x128,  (2, 5, 7, 128, 256, 1, 1, 1, 0, 0, 5, 7, True),            ("relu", "off")),
    ("H2D_64x128",          1, H2D_64x128,  (2, 5, 7, 192, 256, 1, 1, 1, 0, 0, 5, 7, True),            ("relu", "res1")),
    ("H2D_64x128",          1, H2D_64x128,  (2, 5, 7, 320, 256, 1, 1, 1, 0, 0, 5, 7, False),           ("res2",)),
    # H2K_256x256
    ("H2K_256x256",         1, H2_256,      (2, 17, 17, 32, 256, 3, 1, 2, 2, 2, 17, 17, False),        ("d2", "res2")),
    ("H2K_256x256",         1, H2_256,      (2, 17, 17, 32, 512, 3, 1, 1, 1, 1, 17, 17, True),         ("relu", "res1")),
    ("H2K_256x256",         1, H2_256,      (2, 17, 17, 32, 256, 3, 1, 1, 1, 1, 17, 17, True),         ("relu", "off")),
    # H2K_256x128
    ("H2K_256x128",         1, H2_256,      (2, 17, 17, 32, 128, 3, 1, 2, 2, 2, 17, 17, False),        ("d2", "res2")),
    ("H2K_256x128",         1, H2_256,      (2, 17, 17, 32, 384, 3, 1, 1, 1, 1, 17, 17, True),         ("relu", "res1")),
    ("H2K_256x128",         1, H2_256,      (2, 17, 17, 32, 128, 3, 1, 1, 1, 1, 17, 17, True),         ("relu", "off")),
    # H2K_256x128, split-K
    ("H2K_256x128",         2, H2K_FEW,     (2, 17, 17, 96, 256, 3, 1, 2, 2, 2, 17, 17, False),        ("d2", "res2")),
    ("H2K_256x128",         2, H2K_FEW,     (2, 17, 17, 96, 256, 3, 1, 1, 1, 1, 17, 17, True),         ("relu", "res1")),
    ("H2K_256x128",         2, H2K_FEW,     (2, 17, 17, 96, 256, 3, 1, 1, 1, 1, 17, 17, True),         ("relu", "off")),
    # H2K_512x64
    ("H2K_512x64",          1, H2K_512,     (2, 23, 23, 32, 64, 3, 1, 2, 2, 2, 23, 23, False),         ("d2", "res2")),
    ("H2K_512x64",          1, H2K_512,     (2, 23, 23, 32, 64, 3, 1, 1, 1, 1, 23, 23, True),          ("relu", "res1")),
    ("H2K_512x64",          1, H2K_512,     (2, 23, 23, 32, 64, 3, 1, 1, 1, 1, 23, 23, True),          ("relu", "off")),
    # H2K_256x64
    ("H2K_256x64",          1, H2_256,      (2, 17, 17, 32, 64, 3, 1, 2, 2, 2, 17, 17, False),         ("d2", "res2")),
    ("H2K_256x64",          1, H2_256,      (2, 17, 17, 32, 192, 3, 1, 1, 1, 1, 17, 17, True),         ("relu", "res1")),
    ("H2K_256x64",          1, H2_256,      (2, 17, 17, 32, 64, 3, 1, 1, 1, 1, 17, 17, True),          ("relu", "off")),
]


# rows that no selection reaches: the fusions put them in place of a selected row (test_conv_choice.SET_BY_FUSIONS); the
# tests that run them assert the row through ops.last_conv themselves
FUSION_ROWS = {
    "H2KF_256x64": "test_ops.py::test_bottleneck_tail_fused_vs_f64 (C = 64), test_bottleneck_block.py (conv_block_kernel's record)",
    "H2KF_256x128": "test_ops.py::test_bottleneck_tail_fused_vs_f64 (C = 128)",
    "H2KF_256x256": "test_ops.py::test_bottleneck_tail_fused_vs_f64 (C = 256)",
    "H2_STEM": "test_ops.py::test_stem_kernel_vs_two_launches_and_f64 (fuse=True)",
}

# every (row, split-K > 1) pair conv_select (csrc/conv_split.hip) can emit, with the rule that emits it.  Everything else runs
# whole reductions: SPLIT1 (rule_split1: 1), the kw-reuse rows SPLIT3K_* / H2K_256x256 / H2K_256x64 / H2K_512x64 (kwr3 needs
# k3 == 1), H2_64x64 (64-wide n-tiles only for K <= 1024: 1), H2_128x64 / H2_512x64 (rule_h2_n64_*: 1), H2D_* (the double
# stages are added for splitk == 1 only), the exact-f32 rows (no split-K).  True: any factor; a number: that factor alone.
SPLITK_PAIRS = {
    "SPLIT3_256x256": True,      # split3_fit: a 256-row fit carries forced_splitk (ODT_CONV_SPLIT3_FORCE_SPLITK) -> rule_split3
    "SPLIT3_256x128": True,      # the same
    "SPLIT3_256x64": True,       # the same (a forced factor takes the 64-wide layer off the kw-reuse kernel)
    "SPLIT3_128x256": True,      # split3_fit's last branch: too few 128-row tiles -> splitk_for; or the forced factor
    "SPLIT3_128x128": True,      # the same
    "H2_256x256": True,          # rule_h2_256_rows hands the fit's k3 on (forced factors only: a 256-row fit has no other)
    "H2_256x128": True,          # the same
    "H2_128x128": True,          # rule_h2_128_rows: splitk_for(2 * min_tiles3, ...) or the forced factor
    "H2_64x128": 2,              # rule_h2_64_rows: K > 1024 under h2_bm64 == 2, the reduction cut in two
    "H2K_256x128": True,         # rule_h2k_few_rows: splitk_for over the (slice, kh) groups
}

# what a row does NOT take, and why -- every other feature is in the ledger for it (test_conv_rows.py checks both ways)
_KWR = {"s2": "conv_kwr_fits: the kw taps share a staged run of pixels at stride 1 only",
        "cat1": "conv_kwr_fits: no second source (a K-concatenated source belongs to a 1x1 conv, which has no kw taps)",
        "cat2": "conv_kwr_fits: no second source"}
_N64 = {"cat1": "rule_h2_n64_forced / rule_h2_n64_small_tiles pass on a second source: conv_select never emits the row with one",
        "cat2": "the same"}
_H2D = {"s2": "conv_h2d_fits: dense same-size 1x1 convs only (stride 1, no pad)", "d2": "conv_h2d_fits: 1x1 convs have no dilation",
        "cat1": "conv_h2d_fits: in2 == nullptr", "cat2": "conv_h2d_fits: in2 == nullptr"}
_SPLITK = {"cat1": "conv_check_variant: split-K needs a single source (forced_splitk and the rules ask for in2 == nullptr)",
           "cat2": "the same"}
NOT_TAKEN = {      # (row, split-K > 1) -> {feature: reason}
    ("SPLIT3K_256x256", False): _KWR, ("SPLIT3K_256x128", False): _KWR, ("SPLIT3K_256x64", False): _KWR,
    ("H2K_256x256", False): _KWR, ("H2K_256x128", False): _KWR, ("H2K_512x64", False): _KWR, ("H2K_256x64", False): _KWR,
    ("H2K_256x128", True): _KWR,      # (and split-K: a single source anyway)
    ("H2_512x64", False): _N64, ("H2_128x64", False): _N64,
    ("H2D_64x64", False): _H2D, ("H2D_64x128", False): _H2D,
}
NOT_TAKEN.update({(row, True): _SPLITK for row in SPLITK_PAIRS if row != "H2K_256x128"})


def use_env(monkeypatch, env):
  """exactly `env`: every inherited ODT_* variable goes first"""
  for k in [k for k in os.environ if k.startswith("ODT_")]:
    monkeypatch.delenv(k)
  for k, v in env.items():
    monkeypatch.setenv(k, v)


def choice_shape(case, features=()):
  """the ops.CONV_CHOICE_SHAPE values of a ledger case as the stand-alone ops build its record (ranges = 1)"""
  B, H, W, Cin, Cout, k, s, d, pt, pl, Ho, Wo, relu = case
  cin2 = sum(CAT[f][0] for f in features if f in CAT)
  res_mode = 1 if "res1" in features else (2 if "res2" in features else 0)
  return conv_shape(B, H, W, Cin, Cout, k, s, d, pt, pl, Ho, Wo, cin2, res_mode)


def conv_shape(B, H, W, Cin, Cout, k, stride, dil, pad_t, pad_l, Ho, Wo, cin2=0, res_mode=0):
  """the ops.CONV_CHOICE_SHAPE values of an ops.conv2d / ops.conv2d_cat call (dense tensors, recorded ranges).  The entry
  point takes ONE pad: the selection reads the pads of a 1x1 conv only (conv_h2d_fits: none), so unequal ones need k > 1."""
  assert pad_t == pad_l or k > 1
  return [B, H, W, Cin, Cout, k, k, stride, dil, pad_t, Ho, Wo, W, cin2, res_mode, 1, 0, 0]


def assert_row(lib, row, splitk=None):
  """the last stand-alone conv call on `lib` launched exactly `row` (with exactly `splitk`)"""
  got = ops.last_conv(lib)
  assert got["name"] == row, "ran %s, expected %s" % (got["name"], row)
  if splitk is not None:
    assert got["splitk"] == splitk, "ran %s with split-K %d, expected %d" % (row, got["splitk"], splitk)
  return got


def assert_choice_agrees(lib, shape):
  """ops.conv_choice for `shape` under the current knobs == what the last call launched: all eleven fields and the name"""
  want = ops.conv_choice(shape, lib=lib)
  got = ops.last_conv(lib)
  assert got == want, "launched %r, odt_op_conv_choice reports %r for %r" % (got, want, shape)
  return got


_INPUTS = {}


def entry_inputs(case, features):
  """inputs, the float64 result and the magnitude sum  sum |a||w| + |bias| (+ |res|)  of an entry: computed once, shared by the
  backends, never modified"""
  key = (case, features)
  if key in _INPUTS:
    return _INPUTS[key]
  B, H, W, Cin, Cout, k, s, d, pt, pl, Ho, Wo, relu = case
  rng = np.random.default_rng(sum((i + 1) * int(v) for i, v in enumerate(case)) + 1000 * len(features))
  t = {"x": rng.standard_normal((B, H, W, Cin)).astype(F), "b": rng.standard_normal(Cout).astype(F), "res": None, "x2": None}
  cat = [f for f in features if f in CAT]
  f64 = np.float64
  if cat:
    c2, s2 = CAT[cat[0]]
    Hb, Wb = (Ho, Wo) if s2 == 1 else (2 * Ho, 2 * Wo - 1)
    t["x2"] = rng.standard_normal((B, Hb, Wb, c2)).astype(F)
    t["w"] = (rng.standard_normal((Cin, Cout)) * np.sqrt(1.0 / Cin)).astype(F)
    t["w2"] = (rng.standard_normal((c2, Cout)) * np.sqrt(1.0 / c2)).astype(F)
    xs = t["x2"][:, ::s2, ::s2][:, :Ho, :Wo].astype(f64)
    ref = t["x"].astype(f64) @ t["w"].astype(f64) + xs @ t["w2"].astype(f64) + t["b"].astype(f64)
    mag = np.abs(t["x"]).astype(f64) @ np.abs(t["w"]).astype(f64) + np.abs(xs) @ np.abs(t["w2"]).astype(f64) + np.abs(t["b"]).astype(f64)
  else:
    t["w"] = (rng.standard_normal((k, k, Cin, Cout)) * np.sqrt(2.0 / (k * k * Cin))).astype(F)
    ref = torch_conv_nhwc(t["x"], t["w"], t["b"], s, d, pt, pl, Ho, Wo, dtype=f64)
    mag = torch_conv_nhwc(np.abs(t["x"]), np.abs(t["w"]), np.abs(t["b"]), s, d, pt, pl, Ho, Wo, dtype=f64)
  if "res1" in features or "res2" in features:
    rH, rW = (Ho, Wo) if "res1" in features else ((Ho + 1) // 2, (Wo + 1) // 2)
    t["res"] = rng.standard_normal((B, rH, rW, Cout)).astype(F)
    r = t["res"].astype(f64)
    if "res2" in features:
      r = np.repeat(np.repeat(r, 2, 1), 2, 2)[:, :Ho, :Wo]
    ref = ref + r; mag = mag + np.abs(r)
  if relu:
    ref = np.maximum(ref, 0)      # (1-Lipschitz: the bound of the pre-activation value holds)
  t["ref"] = ref; t["mag"] = mag
  for a in t.values():
    if a is not None:
      a.setflags(write=False)
  _INPUTS[key] = t
  return t


def run_entry(lib, case, features):
  """one launch of an entry through the stand-alone op; returns the op's output as it comes back (offset border included)"""
  B, H, W, Cin, Cout, k, s, d, pt, pl, Ho, Wo, relu = case
  t = entry_inputs(case, features)
  cat = [f for f in features if f in CAT]
  if cat:
    return ops.conv2d_cat(t["x"], t["x2"], t["w"], t["w2"], t["b"], stride_b=CAT[cat[0]][1], relu=relu, lib=lib)
  res_mode = 1 if "res1" in features else (2 if "res2" in features else 0)
  return ops.conv2d(t["x"], t["w"], t["b"], s, d, pt, pl, (Ho, Wo), out_off=(1, 1) if "off" in features else (0, 0),
                    res=t["res"], res_mode=res_mode, relu=relu, lib=lib)


BOUND = 5e-6      # test_ops._run_conv's: |y - y64| <= 5e-6 * (sum |a||w| + |bias| (+ |res|)) per element


def error_ratio(y, case, features):
  """max over the elements of |y - y64| / (BOUND * magnitude); the offset border must be exactly zero"""
  t = entry_inputs(case, features)
  if "off" in features:
    assert np.all(y[:, 0] == 0) and np.all(y[:, :, 0] == 0), "the border of the offset output is not zero"
    y = y[:, 1:, 1:]
  assert y.shape == t["ref"].shape and y.dtype == F
  return float((np.abs(y.astype(np.float64) - t["ref"]) / (BOUND * t["mag"])).max())
