"""What the mutable device-resident corpora share (IndexCorpus, QuantizedFrameCorpus): the event that orders
readers and writers on other streams after the last writer, and the host-side checks of row numbers."""
from __future__ import annotations

import numpy as np

from ._dev import is_tensor, stream, to_np, torch


class ResidentRows:
    """Base of a corpus of N rows whose device buffers are rewritten in place.  The subclass provides N."""

    def _mark_ready(self):
        """End of a build or a writer: the buffers are written on the calling thread's stream."""
        self._built_on = stream()
        self._ready = torch().cuda.Event()
        self._ready.record()

    def _wait_ready(self):
        """Entry of every search and writer: ordered after the last writer (an event wait queued on the device,
        no host sync; nothing to wait for on the building stream, or in a corpus never marked)."""
        if self._ready is not None and stream() != self._built_on:
            torch().cuda.current_stream().wait_event(self._ready)

    def _local_rows(self, rows, what: str) -> np.ndarray:
        """Row numbers (sequence, NumPy array or device tensor) as a host int64 array, every one in [0, N):
        IndexError otherwise (raised on the host, before any launch)."""
        name = type(self).__name__
        a = to_np(rows) if is_tensor(rows) else np.asarray(rows)
        a = a.reshape(-1)
        if a.size and a.dtype.kind not in "iu":
            raise TypeError(f"{name}.{what}: row numbers must be integers")
        a = a.astype(np.int64)
        if a.size and (a.min() < 0 or a.max() >= self.N):
            bad = int(a.min()) if a.min() < 0 else int(a.max())
            raise IndexError(f"{name}.{what}: row {bad} outside [0, {self.N})")
        return a

    def _survivors(self, drop: np.ndarray) -> np.ndarray:
        """The rows left when the rows `drop` (duplicates tolerated) go: sorted host int64 row numbers."""
        keep = np.ones(self.N, dtype=bool)
        keep[drop] = False
        return np.flatnonzero(keep)
