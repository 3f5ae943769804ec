"""Segmented hipGraph capture of a training step that may contain collectives, and the warm-up in front of a capture.

A step is captured once and replayed.  A collective reached while capturing (dp.collective) either stays INSIDE the capture
(NERFSIG_CAPTURE_COLLECTIVES=1: RCCL's kernels become graph nodes) or ends the running segment: it is remembered as the eager call
that follows that segment in every replay, and the next segment begins in the same memory pool.  One rank: a single segment.
Both captured training loops (trainer.GraphedWatermarkLoop, stage1.GraphedCleanLoop) and the grid refresh (gridrefresh.DeviceGridRefresh, one
segment) capture through SegmentedCapture and warm up through warm_up; blockgraph.py keeps its own pair of graphs (torch.autograd.grad between them)."""
import gc

import torch

from . import dp


class SegmentedCapture:
    def __init__(self, stream=None, on_boundary=None, after_first=None):
        """stream: the stream to capture on (default: one of this object's own, made at the first capture); a caller that captures more than once
        passes its own -- autograd's accumulation nodes remember the stream they were made on.  on_boundary(): run whenever a segment has ended,
        at a collective and once the capture is over.  after_first(): run by replay() right behind the first segment."""
        self.segments, self.between = [], []
        self.stream, self.on_boundary, self.after_first = stream, on_boundary, after_first

    def _segment_ended(self):
        if self.on_boundary is not None:
            self.on_boundary()

    def capture(self, fn):
        """Capture fn() (no arguments; its tensors are static) on this object's stream.  Returns fn's result (static tensors)."""
        self.segments, self.between = [torch.cuda.CUDAGraph()], []
        open_capture = [True]

        def boundary(coll, last=False):
            self.segments[-1].capture_end()
            self._segment_ended()
            self.between.append(coll)
            if last:                         # the step ends with this collective: no empty segment behind it
                open_capture[0] = False
                return
            g = torch.cuda.CUDAGraph()
            self.segments.append(g)
            g.capture_begin(pool=self.segments[0].pool(), capture_error_mode="thread_local")

        gc.collect()
        torch.cuda.synchronize()
        dp.drain_watchdog()       # (a no-op without an nccl group) nothing of the warm-up's collectives may be left with ProcessGroupNCCL's watchdog thread
        if self.stream is None:
            self.stream = torch.cuda.Stream()
        self.stream.wait_stream(torch.cuda.current_stream())
        prev = dp.set_boundary(boundary)
        try:
            # thread_local: with more than one rank the process group's watchdog thread queries events while we capture; only this thread's calls belong to the capture
            with torch.cuda.stream(self.stream):
                self.segments[0].capture_begin(capture_error_mode="thread_local")
                try:
                    out = fn()
                except BaseException:
                    # fn() raised in the middle of a segment: the stream must not be left capturing (every later launch on it would fail with "operation not
                    # permitted when stream is capturing").  End the open segment, drop everything captured so far, and let the error travel.
                    if open_capture[0]:
                        open_capture[0] = False
                        try:
                            self.segments[-1].capture_end()
                        except Exception:      # noqa: BLE001 -- the capture may already be invalidated by the failing call; the original error is the one to report
                            pass
                    self.segments, self.between = [], []
                    raise
                if open_capture[0]:
                    self.segments[-1].capture_end()
        finally:
            dp.set_boundary(prev)
        torch.cuda.current_stream().wait_stream(self.stream)
        self._segment_ended()
        return out

    def replay(self):
        for i, g in enumerate(self.segments):
            g.replay()
            if i == 0 and self.after_first is not None:
                self.after_first()
            if i < len(self.between):
                self.between[i]()        # the collective between two segments (ordered behind the segment on the current stream)


def warm_up(fn, n, optimizer, params, extra=()):
    """Run fn() n times on a side stream, then undo what they trained: the values of `params` and of the `extra` device tensors (None entries
    are skipped) and the optimiser's state are restored IN PLACE -- a graph captured afterwards holds their addresses -- and state the warm-up
    created goes back to its initial value, zero.  What stays is what the warm-up is for: library handles, lazily created optimiser state,
    loaded modules, algorithm choices, all of which must exist before a capture."""
    kept = [t for t in (*params, *extra) if t is not None]
    with torch.no_grad():
        saved = [t.detach().clone() for t in kept]
        state = {p: {k: v.clone() for k, v in st.items() if torch.is_tensor(v)} for p, st in optimizer.state.items()}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(n):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    with torch.no_grad():
        for t, v in zip(kept, saved):
            t.copy_(v)
        for p, st in optimizer.state.items():
            for k, v in st.items():
                if torch.is_tensor(v):
                    if k in state.get(p, {}):
                        v.copy_(state[p][k])
                    else:
                        v.zero_()
