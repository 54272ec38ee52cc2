"""LoopRecorder - trajectories and tracking-error statistics of a device-resident control loop.

What the reference's closed-loop examples keep in `ee_track`, `target_track` and `q_track` lists and reduce with
`np.linalg.norm(ee - target)` at the end, kept on the device: `record()` is one kernel (engine.loop_trace) that
snapshots the chosen columns into a time-major history and updates per-arm statistics, and it is recordable into an
engine.Plan, so { path_next; OSC; plant_step; recorder.record } replayed with launch_graph(K) returns K ticks of history
and statistics without the host.

    rec = LoopRecorder(rc, B, capacity=1000, columns=("q", "xyz", "err"), stream=s)
    with engine.Plan(0, s) as tick:
        ...
        rec.record(q, dq, u, tgt)
    tick.launch_graph(1000)
    rec.history()["xyz"]      # [T, B, 3]
    rec.stats()["err_rms"]    # [B]
"""
import math

import numpy as np

from . import _abi, engine
from ._lib import DeviceArray


class LoopRecorder:
    """Owns the buffers of engine.loop_trace for B rows of the arm `rc` (a robot_config of this package).

    capacity: history slots (0: statistics only); every: the history keeps every `every`-th tick; columns: names out of
    ("q", "dq", "u", "target", "xyz", "err") - stored in that order whatever order they are named in; ref_frame /
    xyz_offset: the point whose position is `xyz` (as robot_config.Tx); tol: settling tolerance on err; stats: keep the
    per-row statistics; stream: the stream record() and reset() run on.  A history at full batch size is large
    (capacity x B x W values): at 1 M arms keep the statistics and a short or decimated history."""

    def __init__(self, rc, B, capacity=0, every=1, columns=("xyz", "err"), ref_frame="EE", xyz_offset=None, tol=1e-3,
                 stats=True, stream=None):
        B, capacity, every = int(B), int(capacity), int(every)
        if B < 1:
            raise ValueError(f"B={B} < 1")
        if capacity < 0:
            raise ValueError(f"capacity={capacity} < 0")
        if every < 1:
            raise ValueError(f"every={every} < 1")
        if capacity == 0 and not stats:
            raise ValueError("nothing to record: capacity=0 and stats=False")
        if not math.isfinite(float(tol)):
            raise ValueError(f"tol={tol} is not finite")
        if xyz_offset is not None:
            xyz_offset = np.asarray(xyz_offset, dtype=float)
            if xyz_offset.shape != (3,) or not np.isfinite(xyz_offset).all():
                raise ValueError("xyz_offset: three finite values")
        self.rc, self.B, self.capacity, self.every, self.stream = rc, B, capacity, every, stream
        self.n, self.dtype, self.device = rc.N_JOINTS, np.dtype(rc.dtype), rc.device
        columns = tuple(columns)
        mask = _abi.trace_columns_mask(columns)
        if capacity and not mask:
            raise ValueError("a history needs at least one column")
        self.layout, self.W = _abi.trace_layout(mask, self.n)
        self.params = _abi.make_trace_params(rc.frame_id(ref_frame), xyz_offset, every, capacity, mask, tol)
        self._counter = DeviceArray((B,), np.int32, self.device)
        self._history = DeviceArray((capacity, B, self.W), self.dtype, self.device) if capacity else None
        self._stats = DeviceArray((B, 4), np.float64, self.device) if stats else None
        self._settle = DeviceArray((B,), np.int32, self.device) if stats else None
        if self._history is not None:  # all-ones bytes are a NaN in both types: slots never written read as NaN
            engine.check(engine.lib().abrk_memset(self.device, self._history.ptr, 0xFF, self._history.nbytes,
                                                  engine._sp(stream)))
        self.reset()

    def record(self, q, dq, u, target):
        """One tick (inside `with engine.Plan(...)`: recorded).  DeviceArrays [B,n], [B,n], [B,n], [B,6] of the arm's
        dtype; dq / u may be None when their columns are not recorded."""
        engine.loop_trace(self.rc.arm_id, self.n, self.params, q, dq, u, target, self._counter, self._history,
                          self._stats, self._settle, dtype=self.dtype, device=self.device, stream=self.stream)

    def reset(self, rows=None):
        """Restart all rows, or rows [lo, hi): a zero fill of their tick counter, statistics and settling state on the
        recorder's stream (ordered with the ticks enqueued there before and after it)."""
        lo, hi = (0, self.B) if rows is None else (int(rows[0]), int(rows[1]))
        for arr in (self._counter, self._stats, self._settle):
            if arr is not None:
                arr.rows(lo, hi).zero_(self.stream)

    def _ticks(self):
        return self._counter.numpy(self.stream).astype(np.int64)

    def history(self):
        """{column: [T, B, w]} with T = min(capacity, ceil(max(counter) / every)); the slots a row has not written since
        its last reset are NaN."""
        if self._history is None:
            raise ValueError("this recorder keeps no history (capacity=0)")
        ticks = self._ticks()
        filled = np.minimum(self.capacity, -(-ticks // self.every))  # per row
        T = int(filled.max())
        h = self._history.numpy(self.stream)[:T]
        h[np.arange(T)[:, None] >= filled[None, :]] = np.nan
        return {name: h[:, :, o:o + w] for name, (o, w) in self.layout.items()}

    def stats(self):
        """{err_last, err_max, err_min, err_rms, ticks, settle_tick}, each [B].  settle_tick: the tick since which the row
        has stayed within tol, -1 while it is outside.  A row with no tick yet has NaN statistics."""
        if self._stats is None:
            raise ValueError("this recorder keeps no statistics (stats=False)")
        ticks = self._ticks()
        s = self._stats.numpy(self.stream)
        settle = self._settle.numpy(self.stream)
        none = ticks == 0
        out = {k: np.where(none, np.nan, s[:, i]) for i, k in enumerate(("err_last", "err_max", "err_min"))}
        out["err_rms"] = np.sqrt(np.where(none, np.nan, s[:, 3]) / np.maximum(ticks, 1))
        out["ticks"] = ticks
        out["settle_tick"] = settle.astype(np.int64) - 1
        return out

    def device_history(self):
        """the history buffer [capacity, B, W] (None without one); `layout` maps column names to (first column, width)"""
        return self._history

    def device_stats(self):
        """{"stats": [B,4] float64 (err_last, err_max, err_min, err_sumsq), "settle": [B] int32, "counter": [B] int32}"""
        return {"stats": self._stats, "settle": self._settle, "counter": self._counter}
