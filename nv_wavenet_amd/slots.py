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

Requests may also be mel frames, upsampled by the engine (its setUpsampling table) as they are generated, and streamed: a front end
that emits frames while it decodes submits what it has and extends the request as more are written into the same tensor.

    h = stream.submit_mel(mel, frames=0, final=False)   # mel: CUDA tensor [n_cond][capacity]; frames written so far
    stream.extend_mel(h, 12)                            # 12 frames written now (queued or running)
    stream.extend_mel(h, 40, final=True)                # the last of them
    stream.step(2048)                                   # min(2048, headroom) samples: a step never outruns the frames written

A queued streamed request is admitted once it has frames for min(count, its length) samples, so admitting never shortens a step.
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
        self._queue = deque()                          # (handle, features, uid, mel request or None) waiting for a column
        self._running = {}                             # column -> [handle, samples still to come (None: mel, see _mel)]
        self._mel = {}                                 # handle -> [frames, final, column or None, samples delivered] of mel requests
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
        self._queue.append((handle, features, int(uid), None))
        return handle

    def submit_mel(self, mel, uid=None, frames=None, final=True):
        """Queues one mel utterance (mel [n_cond][capacity], CUDA, float32 or float16, its first `frames` -- default all -- written;
        final: no more will come); returns its handle.  uid as for submit."""
        assert mel.dim() == 2, "mel: [n_cond][frames]"
        n = mel.size(1) if frames is None else int(frames)
        assert 0 <= n <= mel.size(1) and (n > 0 or not final)
        handle = self._next_handle
        self._next_handle += 1
        if uid is None:
            uid = self._next_uid
        self._next_uid = max(self._next_uid, int(uid) + 1)
        req = [n, bool(final), None, 0]
        self._mel[handle] = req
        self._queue.append((handle, mel, int(uid), req))
        return handle

    def extend_mel(self, handle, frames, final=False):
        """The first `frames` frames of mel request `handle` are written (queued or running); final: no more will come."""
        req = self._mel[handle]
        assert not req[1] and frames >= req[0], "a final request, or fewer frames than before"
        if req[2] is not None:
            self.engine.slotMelFrames(req[2], frames, final)
        req[0], req[1] = int(frames), bool(final)

    def _ready(self, item, count):
        req = item[3]
        return req is None or req[1] or req[0] * self.engine.upStride >= count      # (a final request: min(count, length) <= length)

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
        the stream was made with pcm=False).  With mel requests the step is min(count, headroom) samples; none (no engine call, {})
        when a running mel request has no frames beyond what it has delivered."""
        if self._mel:
            count = min(count, self.engine.slotsHeadroom())
            if count == 0:
                return {}
        while self._queue and self._free and self._ready(self._queue[0], count):
            col = heapq.heappop(self._free)
            handle, x, uid, req = self._queue.popleft()
            if req is None:
                self.engine.slotStart(col, x, uid)
                self._running[col] = [handle, x.size(1)]
            else:
                self.engine.slotStartMel(col, x, uid, req[0], req[1])
                req[2] = col
                self._running[col] = [handle, None]
        if self._mel and not self._running:
            return {}
        y = np.empty((self.columns, count), dtype=np.int32)
        pcm = np.empty((self.columns, count), dtype=np.int16) if self.pcm else None
        if not self.engine.slotsStep(count, y, pcm):
            raise RuntimeError("slot step of %d samples failed" % count)
        out = {}
        for col in sorted(self._running):
            rec = self._running[col]
            req = self._mel.get(rec[0]) if rec[1] is None else None
            left = rec[1] if req is None else (req[0] * self.engine.upStride - req[3] if req[1] else count)
            n = min(count, left)
            out[rec[0]] = (y[col, :n].copy(), pcm[col, :n].copy() if pcm is not None else None)
            if req is None:
                rec[1] -= n
            else:
                req[3] += n
            if (rec[1] == 0) if req is None else (req[1] and req[3] == req[0] * self.engine.upStride):
                if req is not None:
                    del self._mel[rec[0]]
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
