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

A running request's state is a value (nvw_slot_move / nvw_slot_save / nvw_slot_resume), which the stream uses twice.
When load falls the survivors of a burst are scattered over the batch and every step still launches up to the highest of them:
compact() moves the requests beyond the first 16 * ceil(running / 16) columns into the free columns below, and
SlotStream(..., compact=True) does so in every step, after finished requests have retired and before queued ones are admitted.
suspend() takes a request out -- its column is free for something more urgent, or its engine can be drained -- and resume() puts it
back at the front of the queue of this or any other stream whose engine has the same model and seed; what was delivered before the
suspend is not delivered again.

    state = stream.suspend(h)                           # a SlotState: the blob, the source tensor, uid, samples done
    h2 = other_stream.resume(state)                     # goes on at sample state.done

Draining an engine, rebalancing and checkpointing take many requests at once (nvw_slots_save_list /
nvw_slots_resume_list): suspend_many() saves all the running ones among its handles with one launch into the rows of one buffer --
on the GPU, or in pinned host memory, which the device writes in place --, drain() does so for everything the stream holds, and
resume_many() puts a list of states back, which the admitting step hands to the engine in one call per buffer.  A state can leave the
process: to_bytes() is a small record and the blob, from_bytes() the way back (the source tensor is the caller's to hand over again).

    states = stream.drain(pinned=True)                  # every request, running ones first; the stream is empty afterwards
    data = [st.to_bytes() for st in states]             # ... to a file, to another process
    back = [SlotState.from_bytes(d, src, pinned=True) for d, src in zip(data, sources)]
    handles = other_stream.resume_many(back)            # at the front of the queue, in this order

A request may carry a sampling temperature (nvw_slot_set_temperature): the last step of the network draws from
softmax(logits / T).  It is set when the request is submitted or at any time after -- from the next step on --, and suspend, drain,
resume, compact and to_bytes / from_bytes keep it (a blob holds it in word 10 of its header).

    h = stream.submit(features, temperature=0.8)
    stream.set_temperature(h, 1.1)                      # waiting or running: the samples of the steps that follow

A request may carry a probability floor as well (min-p; nvw_slot_set_min_p): the bins whose tempered probability is
below min_p times that of the most probable bin are not drawn.  It travels as the temperature does (word 11 of a blob's header).
min_p_rows() gives a scoring user the log-probabilities of the distribution such a request was drawn from.

    h = stream.submit(features, temperature=0.8, min_p=0.05)
    stream.set_min_p(h, 0.1)

A request may carry tail cuts (top-k, top-p; nvw_slot_set_top_k, nvw_slot_set_top_p): it is drawn from its top_k most
probable bins, and from the smallest set of most probable bins whose mass reaches top_p; the cuts and the floor intersect.  They
travel as the floor does (words 12 and 13 of a blob's header).  cut_rows() gives a scoring user the log-probabilities of the
distribution such a request was drawn from.

    h = stream.submit(features, top_k=50, top_p=0.9)
    stream.set_top_k(h, 1)                              # greedy from the next step on

A request may carry a prime (nvw_slot_prime): its first n samples are given -- the tail of the previous sentence,
the samples a lost stream had already delivered -- and it is drawn from sample n on.  The forced samples are delivered like the
others.  suspend, drain, resume, compact and to_bytes / from_bytes keep what is left of it.

    h = stream.submit(features, prime=delivered)        # integer tensor [n], values in 0..A-1

Forcing a prime through a column costs one sample of generation per forced sample.  The state behind it can be computed instead
(nvw_prefill_states): a time-parallel pass over the last W samples of the prime writes the blob the column would
have saved after them -- byte for byte --, and the request enters as a resume at sample n.  Its delivery then starts at sample n:
the caller has the forced samples already.

    h = stream.submit(features, prime=delivered, prefill=True)
    state = stream.prefill(features, delivered)         # or the state itself: resume() / resume_many() / to_bytes()

A mel request is prefilled in the same way (nvw_prefill_states_mel): the engine upsamples the samples the state
depends on from the request's own frames, bit for bit as its feed would have.

    h = stream.submit_mel(mel, prime=delivered, prefill=True)
    state = stream.prefill_mel(mel, delivered)          # kind "mel"; score_mel(mel, samples) scores from frames likewise

step() waits for its samples, and nothing the host does between steps depends on them: step_async() issues a step and returns
(DESIGN.md §6e).  The engine delivers each running request's valid samples contiguously into one of two pinned buffers the stream
owns (nvw_slots_step_ragged) and names them at once -- column, length, offset, whether the request ends --, so the bookkeeping of
a step is a few numpy operations over the pieces, whatever the number of columns, and a Python loop only over the requests that
start or end in it.  Two steps may be pending: the GPU generates step k + 1 while the host consumes step k.

    pending = None
    while serving or stream.busy() or pending is not None:
        nxt = stream.step_async(2048) if stream.busy() else None      # step k + 1: issued before step k is waited for
        if pending is not None:
            out = pending.result()                                     # a StepOutput: waits for step k only
            for handle, (samples, pcm) in out.items():                 # views of a pinned buffer: valid until two more steps
                ...                                                    # have been issued (.copy() to keep them)
            for handle in stream.finished():
                ...
        pending = nxt                                                  # (None while the stream is idle)
"""
import heapq
import struct
from collections import deque, namedtuple

import numpy as np


def check_temperature(T):
    """T as the engine takes it (a float32 value, finite, in [2^-10, 2^10]); ValueError otherwise."""
    try:
        t = float(np.float32(T))
    except (TypeError, ValueError):
        raise ValueError("temperature %r is not a number" % (T,))
    if not (2.0 ** -10 <= t <= 2.0 ** 10):      # (a NaN fails both comparisons)
        raise ValueError("temperature %r: finite and in [2^-10, 2^10]" % (T,))
    return t


def check_min_p(p):
    """p as the engine takes it (a float32 value, finite, in [0, 0.5]); ValueError otherwise."""
    try:
        t = float(np.float32(p))
    except (TypeError, ValueError):
        raise ValueError("min_p %r is not a number" % (p,))
    if not (0.0 <= t <= 0.5):      # (a NaN fails both comparisons)
        raise ValueError("min_p %r: finite and in [0, 0.5]" % (p,))
    return t + 0.0                 # (-0.0 is 0.0)


def check_top_k(k, A=None):
    """k as the engine takes it (an integer, 0 <= k, and k <= A where the alphabet is known); ValueError otherwise."""
    try:
        t = int(k)
        whole = t == k
    except (TypeError, ValueError, OverflowError):
        raise ValueError("top_k %r is not an integer" % (k,))
    if not whole or t < 0 or t >= 2**31 or (A is not None and t > A):
        raise ValueError("top_k %r: an integer in [0, A]" % (k,))
    return t


def check_top_p(p):
    """p as the engine takes it (a float32 value, finite, in (0, 1]); ValueError otherwise."""
    try:
        t = float(np.float32(p))
    except (TypeError, ValueError):
        raise ValueError("top_p %r is not a number" % (p,))
    if not (0.0 < t <= 1.0):      # (a NaN fails both comparisons)
        raise ValueError("top_p %r: finite and in (0, 1]" % (p,))
    return t


# A request's sampling: the four values, and what each is when it is off.  The order of the fields is the order of the kinds in the
# engine: words 10 to 13 of a blob's header.
Sampling = namedtuple("Sampling", "temperature min_p top_k top_p")
OFF = Sampling(1.0, 0.0, 0, 1.0)
_SLOT_SETTERS = Sampling("slotSetTemperature", "slotSetMinP", "slotSetTopK", "slotSetTopP")      # of WavenetEngine, per field


def check_sampling(temperature=1.0, min_p=0.0, top_k=0, top_p=1.0, A=None):
    """The four values as the engine takes them, as a Sampling (check_temperature, check_min_p, check_top_k, check_top_p); ValueError
    otherwise."""
    return Sampling(check_temperature(temperature), check_min_p(min_p), check_top_k(top_k, A), check_top_p(top_p))


def cut_rows(rows, top_k=0, top_p=1.0, min_p=0.0):
    """The log-probabilities of the cut, renormalised distribution: rows = log-probabilities [n][A] (or [A]) from any scoring entry
    (at the temperature the samples were drawn at); top_k, top_p, min_p = a value or [n] values each.  With q = exp(rows - max):
    top_k keeps q >= the k-th largest q (ties stay; 0: off), top_p keeps q >= theta, theta the largest value of q whose kept mass
    still reaches top_p times the whole mass (the smallest set of most probable bins whose mass reaches top_p, ties included; 1:
    off), min_p keeps q >= min_p.  The kept set is the intersection -- each cut is defined on the full distribution of the row, not
    on what the others left --; dropped bins read -inf and the kept ones are renormalised by the log of their summed probability
    (float64 inside; the result has the dtype of rows).  numpy in, numpy out; a torch tensor in, a torch tensor on the same device
    out.  This is the distribution a request with those values was drawn from, EXCEPT at boundaries within rounding: the kernel
    compares and sums exp2(fma(z, c, -(m c))) in float32 (see min_p_rows), so a bin whose q is within about 1e-5 (relative) of a
    threshold, or a prefix mass within about 1e-5 of top_p, may fall on the other side there."""
    torch_in = not isinstance(rows, np.ndarray) and hasattr(rows, "detach")
    r = rows.detach().cpu().numpy() if torch_in else np.asarray(rows)
    r64 = np.atleast_2d(r.astype(np.float64))
    n, A = r64.shape
    k = np.asarray(top_k).reshape(-1)
    p = np.asarray(top_p, dtype=np.float64).reshape(-1)
    tau = np.asarray(min_p, dtype=np.float64).reshape(-1)
    if k.size not in (1, n) or k.dtype.kind not in "iu" or not np.all((k >= 0) & (k <= A)):
        raise ValueError("top_k: one integer or one per row, each in [0, %d]" % A)
    if p.size not in (1, n) or not np.all((p > 0.0) & (p <= 1.0)):
        raise ValueError("top_p: one value or one per row, each in (0, 1]")
    if tau.size not in (1, n) or not np.all((tau >= 0.0) & (tau <= 0.5)):
        raise ValueError("min_p: one value or one per row, each in [0, 0.5]")
    k, p, tau = np.broadcast_to(k, (n,)), np.broadcast_to(p, (n,)), np.broadcast_to(tau, (n,))
    rel = r64 - r64.max(axis=1, keepdims=True)
    q = np.exp(rel)
    desc = -np.sort(-q, axis=1)
    rows_i = np.arange(n)
    theta_k = np.where(k > 0, desc[rows_i, np.maximum(k, 1) - 1], 0.0)
    # the mass of the bins >= each distinct value, at every position of the sorted row: the prefix sum up to the LAST bin of a tie
    cum = np.cumsum(desc, axis=1)
    last = np.empty_like(cum)
    last[:, -1] = cum[:, -1]
    for j in range(A - 2, -1, -1):
        last[:, j] = np.where(desc[:, j] == desc[:, j + 1], last[:, j + 1], cum[:, j])
    reach = last >= (p * cum[:, -1])[:, None]
    reach[:, -1] = True
    theta_p = np.where(p < 1.0, desc[rows_i, np.argmax(reach, axis=1)], 0.0)
    thr = np.maximum(np.maximum(theta_k, theta_p), tau)
    keep = q >= thr[:, None]
    with np.errstate(divide="ignore"):
        kept = np.where(keep, q, 0.0)
        out = np.where(keep, rel - np.log(kept.sum(axis=1, keepdims=True)), -np.inf)
    out = out.reshape(r.shape).astype(r.dtype if r.dtype.kind == "f" else np.float64)
    if torch_in:
        import torch
        return torch.from_numpy(out).to(rows.device)
    return out


def min_p_rows(rows, min_p):
    """The log-probabilities of the floored, renormalised distribution: rows = log-probabilities [n][A] (or [A]) from any scoring
    entry (WavenetEngine.scoreSamples(rows=True), at the temperature the samples were drawn at), min_p = the floor, a float or [n]
    values.  A bin stays when rows[t][a] - max_a rows[t][a] >= log(min_p); the others read -inf, and the kept ones are
    renormalised by the log of their summed probability (float64 inside; the result has the dtype of rows).  min_p = 0 returns
    the rows renormalised by their own sum.  numpy in, numpy out; a torch tensor in, a torch tensor on the same device out.
    This is the distribution a request with that floor was drawn from, EXCEPT for bins within rounding of the floor: the kernel
    compares exp2(fma(z, c, -(m c))) in float32, whose exponent carries the rounding of m c, of the fma and -- here -- of the
    scoring pass's own subtraction and scaling: a bin whose rows[t][a] - max differs from log(min_p) by less than a few float32
    ulps of (c max|Za| + max|rows|) -- about 1e-5 at the shipped shapes -- may be kept by one and dropped by the other."""
    torch_in = not isinstance(rows, np.ndarray) and hasattr(rows, "detach")
    r = rows.detach().cpu().numpy() if torch_in else np.asarray(rows)
    r64 = np.atleast_2d(r.astype(np.float64))
    tau = np.asarray(min_p, dtype=np.float64).reshape(-1)
    if tau.size not in (1, r64.shape[0]) or not np.all((tau >= 0.0) & (tau <= 0.5)):
        raise ValueError("min_p: one value or one per row, each in [0, 0.5]")
    rel = r64 - r64.max(axis=1, keepdims=True)
    with np.errstate(divide="ignore"):
        keep = rel >= np.log(tau)[:, None]
        kept = np.where(keep, np.exp(rel), 0.0)
        out = np.where(keep, rel - np.log(kept.sum(axis=1, keepdims=True)), -np.inf)
    out = out.reshape(r.shape).astype(r.dtype if r.dtype.kind == "f" else np.float64)
    if torch_in:
        import torch
        return torch.from_numpy(out).to(rows.device)
    return out


def check_prime(prime, length=None):
    """prime as the engine takes it: a 1-D integer tensor of 1..length values, returned as contiguous int32 (None stays None);
    ValueError otherwise.  The values are clamped into the alphabet by the engine."""
    if prime is None:
        return None
    import torch
    if not isinstance(prime, torch.Tensor) or prime.dim() != 1 or prime.is_floating_point() or prime.dtype == torch.bool:
        raise ValueError("prime: a 1-D integer tensor")
    if prime.numel() < 1 or (length is not None and prime.numel() > length):
        raise ValueError("prime: %d samples for an utterance of %s" % (prime.numel(), length))
    return prime.to(torch.int32).contiguous()


def window_pieces(counter, count, window):
    """The generation launches of a step: (first window row, samples) for samples [counter, counter + count) of a window of
    `window` rows -- one piece, or two where the rows wrap (the split nvWavenetInfer::slotsStep makes)."""
    assert 0 < count <= window
    t = counter % window
    first = min(count, window - t)
    return [(t, first)] if first == count else [(t, first), (0, count - first)]


class SlotState:
    """A suspended request (SlotStream.suspend): blob = the column's state, a CUDA uint8 tensor of WavenetEngine.slotSave (None: the
    request had not started); source = its features or mel tensor; uid; done = samples delivered so far; kind = "features" | "mel";
    frames, final = of a mel request (frames written so far, no more to come); temperature = its sampling temperature (the one in
    the blob's header, word 10; a resume goes on at this attribute's value); prime = its prime (an int32 tensor [n], None: none; a
    resume applies it again when done < n); min_p = its probability floor (word 11 of the blob's header where the engine saved
    the blob; the blobs that prefill and scoring write leave the word zero, and the stream sets the floor after resuming); top_k,
    top_p = its tail cuts (words 12 and 13, likewise)."""

    # to_bytes(): this record, then the blob's bytes (blob_bytes of them; 0: the request had not started)
    RECORD = struct.Struct("<4sIIiiIiI")     # magic, version, kind (0 features, 1 mel), frames, final, uid, done, blob_bytes
    RECORD_BYTES = RECORD.size
    RECORD_MAGIC, RECORD_VERSION = b"NWSS", 1
    BLOB_MAGIC = 0x5453574E                  # the first word of a blob ("NWST"); its words 6 and 7 are done and uid,
    TEMPERATURE_WORD = 10                    # word 10 the temperature as the bits of the float (zero: 1.0)
    MIN_P_WORD = 11                          # word 11 the probability floor likewise (zero: 0.0)
    TOP_K_WORD = 12                          # word 12 top-k, the integer (zero: off)
    TOP_P_WORD = 13                          # word 13 top-p as the bits of the float (zero: 1.0, off)
    # per field of Sampling: (word, off value, the bits of a float32 or the integer itself)
    SAMPLING_WORDS = Sampling((TEMPERATURE_WORD, OFF.temperature, True), (MIN_P_WORD, OFF.min_p, True), (TOP_K_WORD, OFF.top_k, False),
                              (TOP_P_WORD, OFF.top_p, True))
    # to_bytes() of a state with done < n of its prime: behind the blob this record, then the n - done values y[done .. n) (int32)
    PRIME = struct.Struct("<4sII")           # magic, first (= done), count (= n - done)
    PRIME_MAGIC = b"NWSP"

    def __init__(self, blob, source, uid, done, kind, frames=None, final=None, buffer=None, row=0, temperature=1.0, prime=None, min_p=0.0,
                 top_k=0, top_p=1.0):
        self.prime = check_prime(prime)
        self.temperature, self.min_p, self.top_k, self.top_p = check_sampling(temperature, min_p, top_k, top_p)
        self._blob_sampling = self.sampling() if blob is not None else OFF      # (what the engine reads from the header on resume)
        self.blob, self.source, self.uid, self.done, self.kind, self.frames, self.final = blob, source, uid, done, kind, frames, final
        # the blob as a row of a buffer that SlotStream hands to slotsResumeList (suspend_many, drain, from_bytes(pinned=True));
        # None: a blob of its own -- a CUDA tensor of suspend(), resumed by slotResume, or a CPU tensor of from_bytes(), uploaded
        self.buffer, self.row = buffer, row

    def sampling(self, A=None):
        """The four attributes as a Sampling, checked (top_k against the alphabet A where it is known); ValueError otherwise."""
        return check_sampling(self.temperature, self.min_p, self.top_k, self.top_p, A)

    @classmethod
    def _header_words(cls, s):
        """(word, its value) for every field of the Sampling s: zero for a value that is off"""
        return [(word, 0 if v == off else int(np.array([v], dtype="<f4").view("<u4")[0]) if is_float else v)
                for (word, off, is_float), v in zip(cls.SAMPLING_WORDS, s)]

    def to_bytes(self):
        """The state as bytes: RECORD (kind, frames, final, uid, done, the blob's size or 0) followed by the blob.  The source
        tensor is not included.  A blob on the GPU is copied to the host here -- a synchronising copy --, and for a pinned blob
        the call waits for the device to have written it.  A request that had not started has no blob; with a temperature other
        than 1, a floor other than 0 or a cut it carries the 64 bytes of a header alone (magic, uid, done = 0 and words 10 to 13),
        so that the values survive; a blob whose words 11 to 13 are not the state's floor and cuts (a prefilled state) is written
        with them.  A state
        still inside its prime (done < n) ends with the PRIME record and the values y[done .. n); every other state's bytes are
        what they were before primes existed."""
        blob = b""
        s = self.sampling()
        if self.blob is None and s != OFF:
            hdr = np.zeros(16, dtype="<u4")
            hdr[0], hdr[1], hdr[7] = self.BLOB_MAGIC, 1, int(self.uid) & 0xFFFFFFFF
            for word, value in self._header_words(s):
                hdr[word] = value
            blob = hdr.tobytes()
        if self.blob is not None:
            if getattr(self.blob, "is_cuda", False):
                blob = self.blob.cpu().numpy().tobytes()
            else:
                if self.blob.is_pinned():
                    import torch
                    torch.cuda.synchronize()
                blob = self.blob.numpy().tobytes()
            if s[1:] != self._blob_sampling[1:]:      # (word 10 is always the engine's or the pass's own)
                words = np.frombuffer(blob, dtype="<u4").copy()
                for word, value in self._header_words(s)[1:]:
                    words[word] = value
                blob = words.tobytes()
        mel = self.kind == "mel"
        return self.RECORD.pack(self.RECORD_MAGIC, self.RECORD_VERSION, 1 if mel else 0, int(self.frames) if mel else 0,
                                1 if (mel and self.final) else 0, int(self.uid) & 0xFFFFFFFF, int(self.done), len(blob)) + blob + self._prime_bytes()

    def _prime_bytes(self):
        if self.prime is None or self.done >= self.prime.numel():
            return b""
        rest = self.prime[int(self.done):].cpu().numpy().astype("<i4")
        return self.PRIME.pack(self.PRIME_MAGIC, int(self.done), int(rest.size)) + rest.tobytes()

    @classmethod
    def from_bytes(cls, data, source, pinned=False):
        """The state of to_bytes(), with its source tensor (features or mel frames) handed over again.  pinned=True: the blob in
        pinned host memory, which the engine reads in place when the request is admitted (a buffer of its own: one engine call
        per such state); False: a CPU tensor, which the stream uploads then, together with the others of the step (one call).  ValueError for data that is truncated or not a state."""
        import torch
        data = bytes(data)
        if len(data) < cls.RECORD_BYTES:
            raise ValueError("a SlotState record is %d bytes, got %d" % (cls.RECORD_BYTES, len(data)))
        magic, version, kind, frames, final, uid, done, nblob = cls.RECORD.unpack_from(data)
        if magic != cls.RECORD_MAGIC or version != cls.RECORD_VERSION or kind not in (0, 1):
            raise ValueError("not a SlotState record (magic %r, version %d, kind %d)" % (magic, version, kind))
        prime, tail = None, len(data) - cls.RECORD_BYTES - nblob
        if tail >= cls.PRIME.size:
            pmagic, first, count = cls.PRIME.unpack_from(data, cls.RECORD_BYTES + nblob)
            if pmagic != cls.PRIME_MAGIC or first != done or count < 1 or tail != cls.PRIME.size + 4 * count:
                raise ValueError("not a prime record behind the blob (magic %r, first %d, count %d, %d bytes)" % (pmagic, first, count, tail))
            y = np.zeros(first + count, dtype=np.int32)      # (the samples below done are never reached)
            y[first:] = np.frombuffer(data, dtype="<i4", count=count, offset=cls.RECORD_BYTES + nblob + cls.PRIME.size)
            prime, tail = torch.from_numpy(y), 0
        if tail != 0 or (nblob and (nblob < 64 or nblob % 16)):
            raise ValueError("the record announces a blob of %d bytes, %d follow it" % (nblob, len(data) - cls.RECORD_BYTES))
        blob = buffer = None
        values = list(OFF)
        if nblob:
            words = np.frombuffer(data, dtype="<u4", count=16, offset=cls.RECORD_BYTES)
            if int(words[0]) != cls.BLOB_MAGIC or int(words[6]) != done or int(words[7]) != uid:
                raise ValueError("the blob's header does not belong to the record (magic %#x, done %d, uid %d)" % tuple(words[[0, 6, 7]]))
            for i, (word, off, is_float) in enumerate(cls.SAMPLING_WORDS):
                if not is_float:
                    values[i] = int(words[word])
                elif int(words[word]):
                    values[i] = float(words[word:word + 1].view("<f4")[0])
                    if values[i] == off and word != cls.TEMPERATURE_WORD:      # (the bits of 1.0 are a valid temperature word, as in the engine)
                        raise ValueError("word %d of the blob's header holds the bits of %r, which zero stands for" % (word, values[i]))
        s = check_sampling(*values)
        if nblob > 64 or (nblob and done):      # (64 bytes with done = 0: the header alone of a request that had not started)
            host = torch.empty((1, nblob), dtype=torch.uint8, pin_memory=bool(pinned))
            host[0].numpy()[:] = np.frombuffer(data, dtype=np.uint8, count=nblob, offset=cls.RECORD_BYTES)
            blob, buffer = host[0], host if pinned else None
        mel = kind == 1
        return cls(blob, source, uid, done, "mel" if mel else "features", frames if mel else None, bool(final) if mel else None, buffer, 0,
                   prime=prime, **s._asdict())


class StepOutput:
    """What one step delivered (PendingStep.result): per delivering request, in ascending column order, handles[i], offsets[i] and
    lengths[i] (numpy) -- its samples are samples[offsets[i] : offsets[i] + lengths[i]], its PCM the same range of pcm (None when the
    stream was made with pcm=False) --, and finished, the handles whose last sample is in this step.  samples and pcm are views of a
    pinned buffer of the stream, valid until the second step after this one is issued (the stream's two buffers take turns).  out[handle] and out.items() slice lazily."""

    def __init__(self, handles, offsets, lengths, samples, pcm, finished):
        self.handles, self.offsets, self.lengths, self.samples, self.pcm, self.finished = handles, offsets, lengths, samples, pcm, finished
        self._index = None

    def __len__(self):
        return len(self.handles)

    def __contains__(self, handle):
        return self._at(handle) is not None

    def _at(self, handle):
        if self._index is None:
            self._index = {int(h): i for i, h in enumerate(self.handles)}
        return self._index.get(int(handle))

    def _slice(self, i):
        a, b = int(self.offsets[i]), int(self.offsets[i]) + int(self.lengths[i])
        return self.samples[a:b], (self.pcm[a:b] if self.pcm is not None else None)

    def __getitem__(self, handle):
        i = self._at(handle)
        if i is None:
            raise KeyError(handle)
        return self._slice(i)

    def items(self):
        for i, h in enumerate(self.handles):
            yield int(h), self._slice(i)


class PendingStep:
    """A step that has been issued (SlotStream.step_async).  result() waits for its samples -- for nothing else -- and returns its
    StepOutput (the same one every time; a pending step issued before it is collected first); done() asks without waiting."""

    def __init__(self, stream, ticket, buf, total, handles, offsets, lengths, finished):
        self._stream, self._ticket, self._buf, self._total = stream, ticket, buf, total
        self._handles, self._offsets, self._lengths, self._finished = handles, offsets, lengths, finished
        self._out = None

    def done(self):
        return self._out is not None or self._ticket is None or self._stream.engine.slotsDone(self._ticket)

    def result(self):
        if self._out is None:
            st = self._stream
            if self._ticket is not None:
                for earlier in list(st._pending):      # (in the order of issue: the steps before this one are collected first)
                    if earlier is self:
                        break
                    earlier.result()
                st.engine.slotsWait(self._ticket)
                y, pcm = st._bufs[self._buf]
                self._out = StepOutput(self._handles, self._offsets, self._lengths, y[:self._total], pcm[:self._total] if pcm is not None else None,
                                       self._finished)
                st._pending.remove(self)
                st._done.extend(self._finished)
            else:      # (a step that generated nothing: step() returns {} there)
                self._out = StepOutput(self._handles, self._offsets, self._lengths, np.empty(0, np.int32), np.empty(0, np.int16) if st.pcm else None, [])
        return self._out


class SlotStream:
    def __init__(self, engine, window, pcm=True, owns_engine=False, compact=False, prefill=False):
        self.engine = engine
        self._prefill = bool(prefill)                  # what submit(prefill=None) does with a prime
        self.columns = engine.maxBatch
        self.window = int(window)
        self.pcm = pcm
        self._owns = owns_engine
        self._compact = bool(compact)
        engine.slotsBegin(self.window)
        self._free = list(range(self.columns))         # a heap: lowest free column first
        self._queue = deque()                          # (handle, features, uid, mel request or None[, SlotState]) waiting for a column
        self._src = {}                                 # handle -> (source tensor, uid) of the running requests
        self._running = {}                             # column -> [handle, samples still to come (None: mel, see _mel)]
        self._mel = {}                                 # handle -> [frames, final, column or None, samples delivered] of mel requests
        self._prime = {}                               # handle -> prime (int32 tensor) of the requests (queued or running) that carry one
        self._sampling = {}                            # handle -> Sampling of the requests (queued or running) that differ from OFF
        # step_async keeps the per-column counts in arrays instead (one numpy operation per step); _arrays says which of the two
        # forms is current, and the other is brought up to date when the caller changes between step() and step_async()
        self._arrays = False
        self._ch = np.full(self.columns, -1, dtype=np.int64)        # per column: the handle it runs (-1: none) ...
        self._left = np.zeros(self.columns, dtype=np.int64)         # ... a feature request's samples still to come ...
        self._deliv = np.zeros(self.columns, dtype=np.int64)        # ... a mel request's samples delivered
        self._pending = []                             # the steps issued by step_async and not yet collected (at most two)
        self._bufs = [None, None]                      # their pinned outputs: (samples, pcm) numpy views, grown on demand
        self._bufs_keep = [None, None]
        self._last_buf = 1                             # the buffer of the step issued last: the next step takes the other
        self._inflight = set()                         # columns that are endpoints of moves the next step has yet to apply
        self._done = []
        self._next_handle = 0
        self._next_uid = 0

    def prefill(self, features, prime, uid=None, temperature=1.0):
        """The state of the utterance (features, uid, temperature) behind the forced samples `prime` (an integer tensor [n], 1 <= n
        <= samples), computed by the engine's time-parallel pass instead of n samples of generation: a SlotState with done = n whose
        blob is byte for byte the one a column primed with them saves after them.  resume() / resume_many() take it (a prime that
        covers the whole utterance leaves nothing to resume), and it survives to_bytes() / from_bytes().  Nothing is queued, no
        column is touched.  uid: as for submit (default: the next one).  The blob is complete once the engine's stream has run
        the pass; a resume orders itself behind it."""
        assert features.dim() == 2 and features.size(1) > 0, "features: [n_cond][samples]"
        temperature = check_temperature(temperature)
        prime = check_prime(prime, features.size(1))
        if prime is None:
            raise ValueError("prefill needs a prime")
        if uid is None:
            uid = self._next_uid
        self._next_uid = max(self._next_uid, int(uid) + 1)
        y = prime if prime.is_cuda else prime.cuda()
        blobs = self.engine.prefillStates([(y, features, int(uid), temperature)])
        state = SlotState(blobs[0], features, int(uid), int(y.numel()), "features", buffer=blobs, row=0, temperature=temperature)
        state._prefilled_from = y      # (read by the pass in stream order: kept with the state)
        return state

    def score(self, features, samples, temperature=1.0):
        """log softmax(Za_t / temperature)[samples[t]] for every t < n of the utterance `features` [n_cond][>= n] fed the known
        `samples` (an integer tensor [n]) from silence: a float32 CUDA tensor [n] from the engine's time-parallel scoring pass
        (WavenetEngine.scoreSamples).  Nothing is queued, no column is touched: the stream's steps deliver what
        they deliver without it.  Complete once the engine's stream has run the pass."""
        assert features.dim() == 2 and features.size(1) > 0, "features: [n_cond][samples]"
        temperature = check_temperature(temperature)
        y = check_prime(samples, features.size(1))
        if y is None:
            raise ValueError("score needs samples")
        return self.engine.scoreSamples([(y if y.is_cuda else y.cuda(), features, temperature)])[0]

    def score_from(self, state, samples, temperature=None, return_state=False):
        """score() behind a state: `samples` (an integer tensor [m]) are scored as local samples state.done .. state.done + m - 1
        of the SlotState's own source -- features or mel frames by state.kind --, from its blob instead of from silence (no blob:
        the request had not started, from silence): a float32 CUDA tensor [m], bit for bit the tail of score() over the whole
        prefix (WavenetEngine.scoreChunks / scoreChunksMel).  temperature: default the state's.  return_state: also
        a SlotState with done + m whose blob is byte for byte the one a column primed with the samples saves there; it resumes
        like any other and survives to_bytes() / from_bytes().  The given state is left as it is.  Nothing is queued, no column
        is touched.  Complete once the engine's stream has run the pass."""
        import torch
        temperature = check_temperature(state.temperature if temperature is None else temperature)
        mel = state.kind == "mel"
        done = int(state.done) if state.blob is not None else 0
        if mel:
            stride = getattr(self.engine, "upStride", 0)
            if not stride or not self.engine.upsampleRowElems():
                raise ValueError("scoring a mel request needs setUpsampling")
            frames = self._mel_frames(state.source, state.frames, bool(state.final))
            room = frames * stride - done
        else:
            room = state.source.size(1) - done
        y = check_prime(samples, None)
        if y is None or room < 1 or y.numel() > room:
            raise ValueError("score_from: 1 .. %d samples behind the %d done" % (max(room, 0), done))
        y = y if y.is_cuda else y.cuda()
        blob = state.blob
        if blob is not None and not (blob.is_cuda or blob.is_pinned()):
            blob = blob.cuda()                         # (a CPU blob of from_bytes())
        if mel:
            req = (blob, y, state.source, int(state.uid), temperature, frames)
            got = self.engine.scoreChunksMel([req], states=bool(return_state))
        else:
            req = (blob, y, state.source[:, done:done + y.numel()], int(state.uid), temperature)
            got = self.engine.scoreChunks([req], states=bool(return_state))
        if not return_state:
            return got[0]
        logp, blobs = got
        prime = state.prime if state.prime is not None and state.prime.numel() > done + y.numel() else None
        after = SlotState(blobs[0], state.source, int(state.uid), done + int(y.numel()), state.kind, frames=state.frames if mel else None,
                          final=state.final if mel else None, buffer=blobs, row=0, temperature=temperature, prime=prime)
        after.min_p = state.min_p                      # (the pass leaves word 11 of the blob zero: the stream sets the floor after the resume)
        after.top_k, after.top_p = state.top_k, state.top_p      # (... and words 12 and 13)
        after._prefilled_from = (y, blob)              # (read by the pass in stream order: kept with the state)
        return logp[0], after

    def _mel_frames(self, mel, frames, final=True):
        assert mel.dim() == 2, "mel: [n_cond][frames]"
        n = mel.size(1) if frames is None else int(frames)
        assert 0 <= n <= mel.size(1) and (n > 0 or not final)
        return n

    def prefill_mel(self, mel, prime, uid=None, temperature=1.0, frames=None, final=True):
        """prefill() for a mel utterance (mel [n_cond][capacity], its first `frames` -- default all -- written; final: no more will
        come): the engine upsamples the samples the state depends on and runs the time-parallel pass on them
        (WavenetEngine.prefillStatesMel).  Returns a SlotState of kind "mel" with done = n, frames and final
        recorded, whose blob is byte for byte the one a mel column primed with `prime` saves after it.  ValueError, with nothing
        counted, when the engine has no upsampling table or the frames written so far do not cover the prime."""
        stride = getattr(self.engine, "upStride", 0)
        if not stride or not self.engine.upsampleRowElems():
            raise ValueError("prefill of a mel request needs setUpsampling")
        n = self._mel_frames(mel, frames, final)
        temperature = check_temperature(temperature)
        prime = check_prime(prime, None)
        if prime is None:
            raise ValueError("prefill needs a prime")
        if prime.numel() > n * stride:
            raise ValueError("prefill: a prime of %d samples, the %d frames written so far upsample to %d" % (prime.numel(), n, n * stride))
        if uid is None:
            uid = self._next_uid
        y = prime if prime.is_cuda else prime.cuda()
        blobs = self.engine.prefillStatesMel([(y, mel, int(uid), temperature, n)])
        self._next_uid = max(self._next_uid, int(uid) + 1)
        state = SlotState(blobs[0], mel, int(uid), int(y.numel()), "mel", frames=n, final=bool(final), buffer=blobs, row=0, temperature=temperature)
        state._prefilled_from = y      # (read by the pass in stream order: kept with the state)
        return state

    def score_mel(self, mel, samples, temperature=1.0, frames=None):
        """score() for a mel utterance: log softmax(Za_t / temperature)[samples[t]] for every t < n, the features upsampled by the
        engine from the first `frames` (default all) frames of mel [n_cond][capacity] -- bit for bit what score() returns for the
        upsampled features (WavenetEngine.scoreSamplesMel).  Nothing is queued, no column is touched."""
        stride = getattr(self.engine, "upStride", 0)
        if not stride or not self.engine.upsampleRowElems():
            raise ValueError("scoring a mel request needs setUpsampling")
        n = self._mel_frames(mel, frames)
        temperature = check_temperature(temperature)
        y = check_prime(samples, n * stride)
        if y is None:
            raise ValueError("score needs samples")
        return self.engine.scoreSamplesMel([(y if y.is_cuda else y.cuda(), mel, temperature, n)])[0]

    def submit(self, features, uid=None, temperature=1.0, prime=None, prefill=None, min_p=0.0, top_k=0, top_p=1.0):
        """Queues one utterance (features [n_cond][T]); returns its handle.  uid: the Philox counter word of its selectors
        (default: 0, 1, 2, ... in submission order) -- the same features, uid and temperature give the same samples whenever they
        run.  temperature: its samples are drawn from softmax(logits / temperature) (ValueError unless finite and in
        [2^-10, 2^10]).  prime: an integer tensor [n], n <= samples -- its first n samples are these (clamped into 0..A-1) and are
        delivered like the others; it is drawn from sample n on (ValueError for a bad shape or length).  The stream keeps the
        tensor while the request is in it.  prefill (None: the stream's default, False unless it was made with prefill=True): True
        with a prime of n < samples values makes the state behind the prime at once (prefill()) and queues the request as a resume
        at sample n -- its delivery starts there, the forced samples are not delivered again, and the samples from n on are bit
        for bit those of prefill=False; ValueError for a prime that covers the whole utterance.  Without a prime it changes
        nothing.  min_p: its samples are drawn without the bins whose tempered probability is below min_p times that of the most
        probable bin (ValueError unless finite and in [0, 0.5]); forced samples stay forced.  top_k, top_p: its samples are drawn
        from its top_k most probable bins (0: off; 1: greedy) and from the smallest set of most probable bins whose mass reaches
        top_p (1: off), on the tempered distribution, intersected with each other and with the floor (ValueError unless top_k is
        an integer in [0, A] and top_p finite and in (0, 1])."""
        assert features.dim() == 2 and features.size(1) > 0, "features: [n_cond][samples]"
        s = self._check(temperature, min_p, top_k, top_p)
        prime = check_prime(prime, features.size(1))
        if (self._prefill if prefill is None else prefill) and prime is not None:
            if prime.numel() >= features.size(1):
                raise ValueError("prefill: a prime of %d samples leaves nothing of an utterance of %d to generate" % (prime.numel(), features.size(1)))
            state = self.prefill(features, prime, uid, s.temperature)
            state.min_p, state.top_k, state.top_p = s[1:]      # (the pass leaves words 11 to 13 of the blob zero: set after the resume, at admission)
            handle = self._next_handle
            self._next_handle += 1
            self._queue.append((handle, features, int(state.uid), None, state))
            self._note(handle, s)
            return handle
        handle = self._next_handle
        self._next_handle += 1
        if uid is None:
            uid = self._next_uid
        self._next_uid = max(self._next_uid, int(uid) + 1)
        self._queue.append((handle, features, int(uid), None))
        self._note(handle, s)
        if prime is not None:
            self._prime[handle] = prime
        return handle

    def submit_mel(self, mel, uid=None, frames=None, final=True, temperature=1.0, prime=None, prefill=None, min_p=0.0, top_k=0, top_p=1.0):
        """Queues one mel utterance (mel [n_cond][capacity], CUDA, float32 or float16, its first `frames` -- default all -- written;
        final: no more will come); returns its handle.  uid, temperature, min_p, top_k, top_p and prime as for submit; the prime of a request that is
        not final is not bounded by the frames written so far (a forced sample still waits for its frames, as a drawn one).
        prefill (None: the stream's default): True with a prime of n values makes the state behind the prime at once
        (prefill_mel()) and queues the request as a mel resume at sample n -- its delivery starts there, the samples from n on are
        bit for bit those of prefill=False, and extend_mel works as for any queued mel request.  ValueError, before anything is
        queued or counted: the engine has no upsampling table, the frames written so far do not cover the prime, a final
        request's prime covers the whole utterance.  Without a prime it changes nothing."""
        s = self._check(temperature, min_p, top_k, top_p)
        if (self._prefill if prefill is None else prefill) and prime is not None:
            stride = getattr(self.engine, "upStride", 0)
            if not stride or not self.engine.upsampleRowElems():
                raise ValueError("prefill of a mel request needs the engine's upsampling table (setUpsampling)")
            n = self._mel_frames(mel, frames, final)
            prime = check_prime(prime, n * stride if final else None)
            if prime.numel() > n * stride:
                raise ValueError("prefill: a prime of %d samples, the %d frames written so far upsample to %d" % (prime.numel(), n, n * stride))
            if final and prime.numel() >= n * stride:
                raise ValueError("prefill: a prime of %d samples leaves nothing of an utterance of %d to generate" % (prime.numel(), n * stride))
            state = self.prefill_mel(mel, prime, uid, s.temperature, n, final)
            state.min_p, state.top_k, state.top_p = s[1:]      # (as in submit)
            handle = self._next_handle
            self._next_handle += 1
            req = self._mel[handle] = [n, bool(final), None, int(state.done)]
            self._queue.append((handle, mel, int(state.uid), req, state))
            self._note(handle, s)
            return handle
        n = self._mel_frames(mel, frames, final)
        prime = check_prime(prime, n * self.engine.upStride if final else None)
        handle = self._next_handle
        self._next_handle += 1
        if uid is None:
            uid = self._next_uid
        self._next_uid = max(self._next_uid, int(uid) + 1)
        req = [n, bool(final), None, 0]
        self._mel[handle] = req
        self._queue.append((handle, mel, int(uid), req))
        self._note(handle, s)
        if prime is not None:
            self._prime[handle] = prime
        return handle

    def _check(self, temperature, min_p, top_k, top_p):
        return check_sampling(temperature, min_p, top_k, top_p, getattr(self.engine, "A", None))

    def _note(self, handle, s):
        if s != OFF:
            self._sampling[handle] = s
        else:
            self._sampling.pop(handle, None)

    def _column(self, handle):
        """The column of a running request, None for a queued one; KeyError for a handle the stream does not hold."""
        col = self.running().get(handle)
        if col is None and not any(item[0] == handle for item in self._queue):
            raise KeyError(handle)
        return col

    def _set(self, handle, field, value):
        col = self._column(handle)
        if col is not None:
            getattr(self.engine, getattr(_SLOT_SETTERS, field))(col, value)
        self._note(handle, self._sampling.get(handle, OFF)._replace(**{field: value}))

    def _get(self, handle, field):
        self._column(handle)
        return getattr(self._sampling.get(handle, OFF), field)

    def set_temperature(self, handle, temperature):
        """Request `handle` samples at `temperature` from the next step on: a running one through the engine at once (its column's
        value changes with that step's first sample), a waiting one when it is admitted.  KeyError for a handle the stream does
        not hold, ValueError for a bad value -- nothing changes."""
        self._set(handle, "temperature", check_temperature(temperature))

    def temperature(self, handle):
        """The temperature request `handle` (queued or running) samples at."""
        return self._get(handle, "temperature")

    def set_min_p(self, handle, min_p):
        """Request `handle` draws with the probability floor `min_p` from the next step on: a running one through the engine at once
        (its column's value changes with that step's first sample), a waiting one when it is admitted.  KeyError for a handle the
        stream does not hold, ValueError for a bad value -- nothing changes."""
        self._set(handle, "min_p", check_min_p(min_p))

    def min_p(self, handle):
        """The probability floor request `handle` (queued or running) is drawn with."""
        return self._get(handle, "min_p")

    def set_top_k(self, handle, top_k):
        """Request `handle` draws from its `top_k` most probable bins from the next step on (0: off): a running one through the
        engine at once, a waiting one when it is admitted.  KeyError for a handle the stream does not hold, ValueError for a bad
        value -- nothing changes."""
        self._set(handle, "top_k", check_top_k(top_k, getattr(self.engine, "A", None)))

    def set_top_p(self, handle, top_p):
        """Likewise with the nucleus mass `top_p` (1: off)."""
        self._set(handle, "top_p", check_top_p(top_p))

    def top_k(self, handle):
        """Top-k request `handle` (queued or running) is drawn with."""
        return self._get(handle, "top_k")

    def top_p(self, handle):
        """Top-p request `handle` (queued or running) is drawn with."""
        return self._get(handle, "top_p")

    def extend_mel(self, handle, frames, final=False):
        """The first `frames` frames of mel request `handle` are written (queued or running); final: no more will come."""
        req = self._mel[handle]
        assert not req[1] and frames >= req[0], "a final request, or fewer frames than before"
        if req[2] is not None:
            self.engine.slotMelFrames(req[2], frames, final)
        req[0], req[1] = int(frames), bool(final)

    def _ready(self, item, count):
        req = item[3]
        return req is None or req[1] or req[0] * self.engine.upStride - req[3] >= count      # (a final request: min(count, length) <= length)

    def busy(self):
        return bool(self._queue or self._running)

    def waiting(self):
        return len(self._queue)

    def running(self):
        """{handle: column} of the requests in the batch."""
        return {rec[0]: col for col, rec in self._running.items()}

    def compact(self):
        """Packs the running requests into the front of the batch: with n of them, every one in a column at or beyond
        16 * ceil(n / 16) moves into the lowest free column below that bound, the highest source first.  Returns the number of
        moves (0: no engine call); the next step applies them before anything else.  While moves of an earlier call are still
        waiting for that step it does nothing (their columns can be neither source nor destination again): call it again after."""
        if self._inflight:
            return 0
        n = len(self._running)
        bound = 16 * ((n + 15) // 16)
        sources = sorted((c for c in self._running if c >= bound), reverse=True)
        if not sources:
            return 0
        targets = sorted(c for c in self._free if c < bound)
        for src, dst in zip(sources, targets):
            self.engine.slotMove(src, dst)
            rec = self._running[dst] = self._running.pop(src)
            self._ch[dst], self._left[dst], self._deliv[dst] = self._ch[src], self._left[src], self._deliv[src]
            self._ch[src] = -1
            if rec[1] is None:
                self._mel[rec[0]][2] = dst
            self._free.remove(dst)
            self._free.append(src)
            self._inflight.update((src, dst))
        heapq.heapify(self._free)
        return len(sources)

    def suspend(self, handle):
        """Takes request `handle` out of the stream and returns its SlotState; a running request's column is saved and freed, a
        queued one is simply dequeued (an empty state unless it was itself resumed).  The handle is gone; resume() gives a new one.
        A request that compact() has just moved cannot be saved before the next step has applied the move: RuntimeError, and
        nothing has changed."""
        for i, item in enumerate(self._queue):
            if item[0] == handle:
                del self._queue[i]
                return self._dequeued(item)
        col = self.running()[handle]
        if col in self._inflight:
            raise RuntimeError("request %d is being moved to column %d: step once before suspending it" % (handle, col))
        blob, done = self.engine.slotSave(col)      # (first: a refusal leaves the stream as it was)
        return self._stopped(handle, col, blob, done)

    def _dequeued(self, item):
        """The state of a request taken out of the queue (an empty one unless it was itself resumed)."""
        handle, req = item[0], item[3]
        s = self._sampling.pop(handle, OFF)
        prime = self._prime.pop(handle, None)
        if req is not None:
            del self._mel[handle]
        if len(item) > 4:
            if req is not None:
                item[4].frames, item[4].final = req[0], req[1]      # (it may have been extended while it waited)
            item[4].temperature, item[4].min_p, item[4].top_k, item[4].top_p = s      # (... or given other values)
            return item[4]
        if req is None:
            return SlotState(None, item[1], item[2], 0, "features", prime=prime, **s._asdict())
        return SlotState(None, item[1], item[2], 0, "mel", req[0], req[1], prime=prime, **s._asdict())

    def _stopped(self, handle, col, blob, done, buffer=None, row=0):
        """Stops the saved request of column `col` and frees the column; its state."""
        self.engine.slotStop(col)
        rec = self._running.pop(col)
        x, uid = self._src.pop(handle)
        s = self._sampling.pop(handle, OFF)      # (the engine has written the same values into the blob's header)
        prime = self._prime.pop(handle, None)
        heapq.heappush(self._free, col)
        self._ch[col] = -1
        if rec[1] is not None:
            left = int(self._left[col]) if self._arrays else rec[1]
            assert done == x.size(1) - left, (done, x.size(1), left)
            return SlotState(blob, x, uid, done, "features", buffer=buffer, row=row, prime=prime, **s._asdict())
        req = self._mel.pop(handle)
        delivered = int(self._deliv[col]) if self._arrays else req[3]
        assert done == delivered, (done, delivered)
        return SlotState(blob, x, uid, done, "mel", req[0], req[1], buffer, row, prime=prime, **s._asdict())

    def suspend_many(self, handles=None, pinned=False):
        """suspend() for a list of requests (None: all of them, running ones first, each group in handle order), with ONE engine
        save for the running ones among them: their blobs are the rows of one buffer -- on the GPU, or with pinned=True in pinned
        host memory, written in place by the device (complete once the stream has got there: to_bytes() waits for it).  Queued
        requests are dequeued as suspend() does.  Returns the SlotStates in the order of `handles`.  KeyError for a handle the
        stream does not hold, ValueError for one named twice, RuntimeError if one is being moved by a compact() whose step has not
        been issued -- all before anything has changed.  Works with steps pending, as suspend() does."""
        running = self.running()
        queued = {item[0]: item for item in self._queue}
        if handles is None:
            handles = sorted(running) + sorted(queued)
        handles = [int(h) for h in handles]
        if len(set(handles)) != len(handles):
            raise ValueError("a handle is named twice")
        for h in handles:
            if h not in running and h not in queued:
                raise KeyError(h)
            if h in running and running[h] in self._inflight:
                raise RuntimeError("request %d is being moved to column %d: step once before suspending it" % (h, running[h]))
        saving = [h for h in handles if h in running]
        states = {}
        if saving:
            cols = [running[h] for h in saving]
            blobs, saved = self.engine.slotsSaveList(cols, pinned=pinned)      # (first: a refusal leaves the stream as it was)
            for i, (h, col) in enumerate(zip(saving, cols)):
                states[h] = self._stopped(h, col, blobs[i], int(saved["done"][i]), blobs, i)
        if len(saving) < len(handles):
            self._queue = deque(item for item in self._queue if item[0] not in set(handles))
            for h in handles:
                if h in queued:
                    states[h] = self._dequeued(queued[h])
        return [states[h] for h in handles]

    def drain(self, pinned=False):
        """Suspends everything the stream holds (suspend_many(None)): the running requests in handle order, then the queued ones in
        handle order.  Afterwards busy() is false and every column is free (the stops are applied by the next step, or dropped by
        close())."""
        return self.suspend_many(None, pinned=pinned)

    def resume_many(self, states):
        """resume() for a list: the states go to the FRONT of the queue in the order given; returns their handles in that order.
        Every blob's size is checked before any state is queued (ValueError, nothing changed).  States whose blobs are rows of
        one buffer (suspend_many, drain) and that a step admits together reach the engine in ONE call, and so do the CPU blobs of
        from_bytes(pinned=False), uploaded together; a from_bytes(pinned=True) state is a pinned buffer of its own, read in
        place, and costs an engine call each -- after a trip through bytes, pinned=False is the path that batches."""
        states = list(states)
        for state in states:
            if hasattr(state.blob, "numel") and state.blob.numel() != self.engine.slotStateBytes():
                raise ValueError("a state of %d bytes, this engine's are %d: another shape or precision" % (state.blob.numel(), self.engine.slotStateBytes()))
        return [self.resume(state) for state in reversed(states)][::-1]

    def resume(self, state):
        """Queues a suspended request at the FRONT (of this stream, or of another whose engine has the same model and seed); returns
        its handle here.  It goes on at sample state.done: nothing delivered before the suspend comes again.  A streamed mel
        request can be extended as before (extend_mel with the new handle).  ValueError, with nothing queued, for a blob whose
        size is not this engine's.  What only the engine can see -- a blob of another model of the same size, a corrupted
        header, a source shorter than `done` -- is refused by the step that admits the request: that step raises ValueError after
        the stream has already booked its admissions, and the stream is to be closed (the engine itself is unchanged by a refused
        list and can be drained)."""
        if hasattr(state.blob, "numel") and state.blob.numel() != self.engine.slotStateBytes():
            raise ValueError("a state of %d bytes, this engine's are %d: another shape or precision" % (state.blob.numel(), self.engine.slotStateBytes()))
        s = state.sampling(getattr(self.engine, "A", None))      # (against this engine's alphabet, before anything is queued)
        handle = self._next_handle
        self._next_handle += 1
        self._next_uid = max(self._next_uid, int(state.uid) + 1)
        req = None
        if state.kind == "mel":
            req = self._mel[handle] = [int(state.frames), bool(state.final), None, int(state.done)]
        self._queue.appendleft((handle, state.source, int(state.uid), req, state))
        self._note(handle, s)
        if state.prime is not None and state.done < state.prime.numel():      # (still inside it: applied again when it is admitted)
            self._prime[handle] = state.prime
        return handle

    def _use_arrays(self, on):
        """Brings the form of the per-column counts that the caller now uses up to date (a loop over the running columns, made
        when the caller changes between step() and step_async(), not per step)."""
        if on == self._arrays:
            return
        for col, rec in self._running.items():
            req = self._mel[rec[0]] if rec[1] is None else None
            if on:
                self._ch[col] = rec[0]
                self._left[col] = rec[1] if req is None else 0
                self._deliv[col] = req[3] if req is not None else 0
            elif req is None:
                rec[1] = int(self._left[col])
            else:
                req[3] = int(self._deliv[col])
        self._arrays = on

    def _admit(self, count):
        """Queued requests into free columns, lowest first, while the head of the queue is ready for a step of `count` samples."""
        listed = []      # (column, state, source, samples | frames, final | None) of the resumes that go to the engine as lists
        primed = []      # (column, handle) of the admitted requests that carry a prime
        wanted = []      # (column, Sampling, what the start or the resume leaves) likewise, where the two differ: a start leaves OFF, a
                         # resume words 10 to 13 of the blob (11 to 13 zero in a prefilled or scored one)
        while self._queue and self._free and self._ready(self._queue[0], count):
            col = heapq.heappop(self._free)
            item = self._queue.popleft()
            handle, x, uid, req = item[:4]
            state = item[4] if len(item) > 4 else None
            blob = state.blob if state is not None else None
            # a row of a shared buffer, or a CPU tensor still to be uploaded: by list; a CUDA blob of its own (suspend()): singly
            by_list = blob is not None and (state.buffer is not None or not getattr(blob, "is_cuda", True))
            self._src[handle] = (x, uid)
            if handle in self._prime:
                primed.append((col, handle))
            s, had = self._sampling.get(handle, OFF), (state._blob_sampling if blob is not None else OFF)
            if s != had:
                wanted.append((col, s, had))
            if req is None:
                if blob is None:
                    self.engine.slotStart(col, x, uid)
                elif by_list:
                    listed.append((col, state, x, x.size(1), None))
                else:
                    self.engine.slotResume(col, blob, x)
                self._running[col] = [handle, x.size(1) - (state.done if blob is not None else 0)]
            else:
                if blob is None:
                    self.engine.slotStartMel(col, x, uid, req[0], req[1])
                elif by_list:
                    listed.append((col, state, x, req[0], bool(req[1])))
                else:
                    self.engine.slotResumeMel(col, blob, x, req[0], req[1])
                req[2] = col
                self._running[col] = [handle, None]
            if self._arrays:
                self._ch[col] = handle
                self._left[col] = self._running[col][1] if req is None else 0
                self._deliv[col] = req[3] if req is not None else 0
        if listed:
            self._resume_listed(listed)
        # start, then set (the engine applies both at the step that follows): every temperature, every floor, then the cuts by column
        order = [(f, it) for f in ("temperature", "min_p") for it in wanted] + [(f, it) for it in wanted for f in ("top_k", "top_p")]
        for field, (col, s, had) in order:
            if getattr(s, field) != getattr(had, field):
                getattr(self.engine, getattr(_SLOT_SETTERS, field))(col, getattr(s, field))
        for col, handle in primed:   # (start or resume, then prime)
            self.engine.slotPrime(col, self._prime[handle])

    def _resume_listed(self, listed):
        """One slotsResumeList call per run of consecutive rows of a shared buffer, in the order admitted (after drain() and
        resume_many(): one call per buffer); the CPU blobs of from_bytes() are uploaded together first, as the rows of one buffer."""
        host = [it for it in listed if it[1].buffer is None]
        if host:
            import torch
            up = torch.stack([it[1].blob for it in host]).cuda()
            for i, it in enumerate(host):
                it[1].blob, it[1].buffer, it[1].row = up[i], up, i
        run = []
        for it in listed + [None]:
            if run and (it is None or it[1].buffer is not run[-1][1].buffer or it[1].row != run[-1][1].row + 1):
                first = run[0][1]
                self.engine.slotsResumeList([r[0] for r in run], first.buffer[first.row:first.row + len(run)], [r[2] for r in run],
                                            [r[3] for r in run], [r[4] for r in run])
                run = []
            run.append(it)

    def step(self, count):
        """Admits waiting requests into free columns, generates `count` samples of every column and returns {handle: (samples, pcm)}
        with this step's samples of every request that ran (numpy int32 / int16, at most `count`, fewer at its end; pcm None when
        the stream was made with pcm=False).  With mel requests the step is min(count, headroom) samples; none (no engine call, {})
        when a running mel request has no frames beyond what it has delivered.  Not while steps of step_async are pending."""
        if self._pending:
            raise RuntimeError("%d pending steps: collect them (PendingStep.result) before a synchronous step" % len(self._pending))
        self._use_arrays(False)
        if self._mel:
            count = min(count, self.engine.slotsHeadroom())
            if count == 0:
                return {}
        if self._compact:
            self.compact()
        self._admit(count)
        if self._mel and not self._running:
            return {}
        y = np.empty((self.columns, count), dtype=np.int32)
        pcm = np.empty((self.columns, count), dtype=np.int16) if self.pcm else None
        if not self.engine.slotsStep(count, y, pcm):
            raise RuntimeError("slot step of %d samples failed" % count)
        self._inflight.clear()
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
                del self._src[rec[0]]
                self._sampling.pop(rec[0], None)
                self._prime.pop(rec[0], None)
                self.engine.slotStop(col)
                heapq.heappush(self._free, col)
                self._done.append(rec[0])
        return out

    def _retire(self, col):
        """The request of column `col` has had its last sample issued: the column stops at the next step and is free."""
        handle = self._running.pop(col)[0]
        self._mel.pop(handle, None)
        self._sampling.pop(handle, None)
        self._prime.pop(handle, None)
        del self._src[handle]
        self._ch[col] = -1
        self.engine.slotStop(col)
        heapq.heappush(self._free, col)
        return handle

    def step_async(self, count):
        """step(), without waiting for the samples: compacts, admits, issues the step, retires what it finishes and returns a
        PendingStep whose result() is the step's StepOutput.  At most two steps may be pending; a third raises RuntimeError before
        anything has changed.  Steps take the stream's two pinned buffers by turns, so a StepOutput's views stay valid until the
        second step after its own has been issued, whether or not steps are pending in between.  suspend, resume, compact and
        extend_mel work with steps pending (they are ordered on the engine's stream, and what a request has done is the host's
        knowledge); with mel requests the step is min(count, headroom) samples, the headroom counted from the frames announced and
        the samples issued, not from what has arrived.  finished() reports a request once the step carrying its last sample has
        been collected."""
        if len(self._pending) >= 2:
            raise RuntimeError("two steps are pending: collect one (PendingStep.result) before issuing a third")
        self._use_arrays(True)
        empty = np.empty(0, dtype=np.int64)
        if self._mel:
            count = min(count, self.engine.slotsHeadroom())
            if count == 0:
                return PendingStep(self, None, None, 0, empty, empty, empty, [])
        if self._compact:
            self.compact()
        self._admit(count)
        if self._mel and not self._running:
            return PendingStep(self, None, None, 0, empty, empty, empty, [])
        buf = self._last_buf ^ 1      # (never the buffer of a pending step: at most one is pending here, and it was issued last)
        need = len(self._running) * ((count + 7) & ~7)
        if self._bufs[buf] is None or self._bufs[buf][0].size < need:
            keep = self.engine.slotsPinned(max(need, 8), self.pcm)
            self._bufs_keep[buf] = keep
            self._bufs[buf] = tuple(a.numpy() if hasattr(a, "numpy") and not isinstance(a, np.ndarray) else a for a in keep)
        y, pcm = self._bufs_keep[buf]
        total, pieces, ticket = self.engine.slotsStepRagged(count, y, pcm)
        self._last_buf = buf
        self._inflight.clear()
        slots = pieces["slot"]
        handles = self._ch[slots]
        self._left[slots] -= pieces["n"]
        self._deliv[slots] += pieces["n"]
        finished = [self._retire(int(col)) for col in slots[pieces["finished"] != 0]]
        step = PendingStep(self, ticket, buf, total, handles, pieces["offset"].copy(), pieces["n"].astype(np.int64), finished)
        self._pending.append(step)
        return step

    def finished(self):
        """Handles that have delivered their last sample since the previous call (each exactly once)."""
        done, self._done = self._done, []
        return done

    def close(self):
        for step in list(self._pending):
            step.result()
        self.engine.slotsEnd()
        if self._owns:
            self.engine.close()
