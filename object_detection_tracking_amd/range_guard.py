"""The fp16x2 range guard of an engine built with ``conv_split_family = "auto"`` (the default).

The fp16x2 kernels scale each tensor by one power of two, which assumes its useful content within 2^17 of its maximum.  The
guard puts the engine's first forward(s) through a bf16x3-only twin engine (no range assumption) as well and moves the
engine to the twin's handle when their pyramid / RPN tensors differ by more than f32 rounding level.  On fp16x2 it keeps
watch: when a tensor's recorded |max| has grown past ``watch_ratio`` times the level the last comparison accepted
(odt_range_health: a scene cut, an exposure change), the comparison is armed again for the next forward."""
import numpy as np

from ._lib import OdtError

AUTO_TAPS = ("p2", "p3", "p4", "p5", "p6", "rpn2", "rpn3", "rpn4", "rpn5", "rpn6")      # (readable after a forward in arena mode too)
MAX_DEFERRED = 16


class RangeGuard(object):

  def __init__(self, config, make_twin):
    self.frames = int(getattr(config, "conv_split_auto_frames", 1) or 1)      # forwards compared per arming
    self.tolerance = float(getattr(config, "conv_split_auto_tol", 2e-5))
    self.watch_ratio = float(getattr(config, "conv_split_auto_watch_ratio", 8.0))
    self.make_twin = make_twin       # () -> a bf16x3-only engine of the same plan (holds config and weights); None: not watching
    self.twin = None                 # the live bf16x3 engine between its first comparison and finish()
    self.chosen = 2                  # conv_split_family the engine runs: 2 (fp16x2) | 3 (bf16x3, for good)
    self.pending = self.frames       # comparisons still to run
    self.checks = []                 # [{"max_rel_diff", "tensor"}] per comparison
    self.deferred = 0                # calls skipped because a ticket was outstanding
    self.incomplete = False          # gave up after MAX_DEFERRED of them
    self.rearmed = 0
    self.watch = None                # the last odt_range_health reading
    self.rebase = False              # armed by the watch: a comparison that keeps fp16x2 accepts the new maxima

  def due(self):
    return self.pending > 0 and self.chosen == 2

  def close(self):
    if self.twin is not None:
      self.twin.close()
      self.twin = None

  def finish(self, incomplete=False):
    self.close()
    if self.chosen == 3 or incomplete:
      self.make_twin = None          # (nothing left to compare: the engine IS the bf16x3 engine, or the guard gave up)
    if incomplete:
      self.incomplete = True
      self.pending = 0

  def calibrate(self, engine, run):
    """One comparison, when one is due: ``run(e)`` puts the caller's input through engine ``e`` (blocking).  ``engine``
    and the twin see the same input; if any pyramid / RPN tensor differs by more than the tolerance (relative to the
    tensor's |max|), ``engine`` continues on the twin's handle.  Returns True when it changed handles.

    Never while a ticket is outstanding: the blocking forward would overwrite the single device output buffers under
    the ticket's copy, and a ticket cannot follow the engine to another handle.  Such calls are skipped (counted in
    report()); after MAX_DEFERRED of them the guard gives up loudly in report() instead of holding the twin forever."""
    if not self.due():
      return False
    if engine._ticket_want:
      self.deferred += 1
      if self.deferred >= MAX_DEFERRED:
        self.finish(incomplete=True)
      return False
    if self.twin is None:
      self.twin = self.make_twin()
      self.twin.set_source_size(engine.src_height, engine.src_width)
    twin = self.twin
    run(engine); run(twin)
    worst, where = 0.0, None
    for name in AUTO_TAPS:
      try:
        x, y = engine.tap(name), twin.tap(name)
      except OdtError:
        continue
      d = float(np.abs(x - y).max() / max(1e-30, float(np.abs(y).max())))
      if not np.isfinite(d):
        d = float("inf")
      if d > worst:
        worst, where = d, name
    self.checks.append({"max_rel_diff": worst, "tensor": where})
    self.pending -= 1
    swapped = worst > self.tolerance
    if swapped:
      engine.take_handle(twin)
      self.chosen = 3
    if self.chosen == 3 or self.pending <= 0:
      self.finish()
      if self.chosen == 2 and self.rebase:
        self.rebase = False
        engine.range_health(rebase=True)
    return swapped

  def after_forward(self, engine):
    """The continuous half: behind every forward / collect / synchronize while the engine runs the fp16x2 kernels."""
    if self.chosen != 2 or self.pending > 0 or self.incomplete or self.make_twin is None:
      return
    self.watch = engine.range_health()
    if self.watch["worst_growth"] > self.watch_ratio:
      self.pending = self.frames     # the next forward also runs on a bf16x3 twin (rebuilt: calibrate)
      self.rearmed += 1
      self.deferred = 0
      self.rebase = True

  def report(self):
    """(describe()["conv_split_family_auto"], describe()["range_guard"])."""
    return ({"chosen": "bf16x3 (family 3)" if self.chosen == 3 else "fp16x2 (family 2)",
             "calibration_forwards_left": max(0, self.pending) if self.chosen == 2 else 0,
             "tolerance": self.tolerance, "checks": list(self.checks),
             "calls_skipped_with_tickets_outstanding": self.deferred, "incomplete": self.incomplete,
             "watch": self.watch, "watch_ratio": self.watch_ratio, "rearmed": self.rearmed},
            "conv_split_family = \"auto\" (default): fp16x2 kernels checked against a bf16x3-only twin handle on the "
            "first forward(s), re-armed whenever a tensor's recorded |max| has grown past watch_ratio times the accepted "
            "level (odt_range_health)" + ("; GAVE UP: every call so far had tickets outstanding" if self.incomplete else ""))
