"""SlotStream: continuous batching on an engine in slot mode (include/nv_wavenet_c.h, nvw_slots_*).

Requests -- one utterance's upsampled features each -- arrive one at a time with different lengths.  Each runs in a column of the
engine's batch from the step it is admitted at until its last sample; its samples do not depend on the column, the step or the other
columns ("Slot mode").  Requests beyond the number of columns wait in a FIFO; a freed column is reused lowest-first, so
the columns in use stay packed at the front of the batch and the launches cover as few tiles as possible.

    stream = SlotStream(engine, window=4096)         # engine: a WavenetEngine with its conditioning weights and seed set
    h = stream.submit(features)                      # CUDA tensor [n_cond][T], float32 or float16
    while stream.busy():
        for handle, (samples, pcm) in stream.step(2048).items():
            ...                                      # this step's samples of every running request
        for handle in stream.finished():
            ...                                      # each finished request once
"""
import heapq
from collections import deque

import numpy as np


def window_pieces(counter, count, window):
    """The generation launches of a step: (first window row, samples) for samples [counter, counter + count) of a window of
    `window` rows -- one piece, or two where the rows wrap (the split nvWavenetInfer::slotsStep makes)."""
    assert 0 < count <= window
    t = counter % window
    first = min(count, window - t)
    return [(t, first)] if first == count else [(t, first), (0, count - first)]


class SlotStream:
    def __init__(self, engine, window, pcm=True, owns_engine=False):
        self.engine = engine
        self.columns = engine.maxBatch
        self.window = int(window)
        self.pcm = pcm
        self._owns = owns_engine
        engine.slotsBegin(self.window)
        self._free = list(range(self.columns))         # a heap: lowest free column first
        self._queue = deque()                          # (handle, features, uid) waiting for a column
        self._running = {}                             # column -> [handle, samples still to come]
        self._done = []
        self._next_handle = 0
        self._next_uid = 0

    def submit(self, features, uid=None):
        """Queues one utterance (features [n_cond][T]); returns its handle.  uid: the Philox counter word of its selectors
        (default: 0, 1, 2, ... in submission order) -- the same features and uid give the same samples whenever they run."""
        assert features.dim() == 2 and features.size(1) > 0, "features: [n_cond][samples]"
        handle = self._next_handle
        self._next_handle += 1
        if uid is None:
            uid = self._next_uid
        self._next_uid = max(self._next_uid, int(uid) + 1)
        self._queue.append((handle, features, int(uid)))
        return handle

    def busy(self):
        return bool(self._queue or self._running)

    def waiting(self):
        return len(self._queue)

    def running(self):
        """{handle: column} of the requests in the batch."""
        return {rec[0]: col for col, rec in self._running.items()}

    def step(self, count):
        """Admits waiting requests into free columns, generates `count` samples of every column and returns {handle: (samples, pcm)}
        with this step's samples of every request that ran (numpy int32 / int16, at most `count`, fewer at its end; pcm None when
        the stream was made with pcm=False)."""
        while self._queue and self._free:
            col = heapq.heappop(self._free)
            handle, x, uid = self._queue.popleft()
            self.engine.slotStart(col, x, uid)
            self._running[col] = [handle, x.size(1)]
        y = np.empty((self.columns, count), dtype=np.int32)
        pcm = np.empty((self.columns, count), dtype=np.int16) if self.pcm else None
        if not self.engine.slotsStep(count, y, pcm):
            raise RuntimeError("slot step of %d samples failed" % count)
        out = {}
        for col in sorted(self._running):
            rec = self._running[col]
            n = min(count, rec[1])
            out[rec[0]] = (y[col, :n].copy(), pcm[col, :n].copy() if pcm is not None else None)
            rec[1] -= n
            if rec[1] == 0:
                del self._running[col]
                self.engine.slotStop(col)
                heapq.heappush(self._free, col)
                self._done.append(rec[0])
        return out

    def finished(self):
        """Handles that have delivered their last sample since the previous call (each exactly once)."""
        done, self._done = self._done, []
        return done

    def close(self):
        self.engine.slotsEnd()
        if self._owns:
            self.engine.close()
