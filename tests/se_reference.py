"""Reference side of the SE-ResNet tests (model version 6): the literal restatement of the reference's bottleneck with
use_se (nn.py:459-521), composed from the oracle's own dense ops, and a context manager that runs an OracleModel on it.
A helper module, not a conftest: the tests import it by name."""
import contextlib

import torch

import oracle.graph as G


def se_bottleneck(x, weights, pre, ch_out, stride, dilation):
  """reference nn.py:459-521 with use_se=True (+ shortcut nn.py:551-566, ReLU nn.py:587): after conv3 + BN
  squeeze = sigmoid(relu(mean_HW(l) . fc1/W + fc1/b) . fc2/W + fc2/b), l = l * squeeze -- the LITERAL mean of conv3's
  output, not the folded form the product evaluates."""
  sc = x
  l = torch.relu(G.batch_norm(G.conv2d(x, weights, pre + "/conv1"), weights, pre + "/conv1/bn"))
  if stride == 2:
    l = G.pad_tl(l)
    l = G.conv2d(l, weights, pre + "/conv2", stride=2, padding="VALID", dilation=dilation)
    l = torch.relu(G.batch_norm(l, weights, pre + "/conv2/bn"))
    if dilation != 1:
      l = G.pad_tl(l)
  else:
    l = G.conv2d(l, weights, pre + "/conv2", dilation=dilation)
    l = torch.relu(G.batch_norm(l, weights, pre + "/conv2/bn"))
  l = G.batch_norm(G.conv2d(l, weights, pre + "/conv3"), weights, pre + "/conv3/bn")
  squeeze = l.mean(dim=(2, 3))                                                      # GlobalAvgPooling, [B, 4 ch]
  squeeze = torch.relu(squeeze @ G._w(weights, pre + "/fc1/W") + G._w(weights, pre + "/fc1/b"))
  squeeze = torch.sigmoid(squeeze @ G._w(weights, pre + "/fc2/W") + G._w(weights, pre + "/fc2/b"))
  l = l * squeeze[:, :, None, None]
  if sc.shape[1] != ch_out * 4:
    if stride == 2:
      sc = sc[:, :, :-1, :-1]
      sc = G.conv2d(sc, weights, pre + "/convshortcut", stride=2, padding="VALID")
    else:
      sc = G.conv2d(sc, weights, pre + "/convshortcut")
    sc = G.batch_norm(sc, weights, pre + "/convshortcut/bn")
  return torch.relu(l + sc)


@contextlib.contextmanager
def se_oracle():
  """While active, oracle.graph's backbone runs se_bottleneck instead of bottleneck."""
  saved = G.bottleneck
  G.bottleneck = se_bottleneck
  try:
    yield
  finally:
    G.bottleneck = saved
