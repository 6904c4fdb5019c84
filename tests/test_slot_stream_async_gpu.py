"""GPU test of SlotStream.step_async (`-m gpu`): one seeded random service -- more requests than columns, feature
requests and streamed mel requests of mixed lengths whose frames are appended between steps, compact=True, one suspend whose
request resumes on a second stream -- runs once with step() and once with step_async() two deep.  Per request the concatenated
samples and PCM must be identical; finished() yields every handle exactly once; a third pending step raises and changes nothing."""
import numpy as np
import pytest
import torch

from nv_wavenet_amd.slots import SlotStream
from test_slots_deliver_gpu import STRIDE, _inputs
from test_slots_gpu import _engine

pytestmark = pytest.mark.gpu

COLUMNS, REQUESTS, CHUNK = 20, 45, 16


def _stream(case, m, w, t, window, columns):
    e = _engine(case, t, 16, "wg", w, m["cond_b"], columns)
    e.setUpsampling(m["up_w"].astype(np.float16).astype(np.float32), m["up_b"], STRIDE)
    return SlotStream(e, window, compact=True, owns_engine=True)


def _service(pipelined):
    case, m, x, w, t, W = _inputs("edge", 16)
    s = case.shape
    frames = s.N // STRIDE
    xg = torch.from_numpy(x).cuda()
    melg = torch.from_numpy(m["features"]).cuda()
    st, st2 = _stream(case, m, w, t, W, COLUMNS), _stream(case, m, w, t, W, 4)
    rng = np.random.default_rng(17)
    reqs = {}                   # request -> dict(stream, handle, kind, ...)
    got = {r: [] for r in range(REQUESTS)}
    finished = {r: 0 for r in range(REQUESTS)}
    for r in range(REQUESTS):
        if r % 3 == 1:          # a streamed mel request: some frames now, the rest appended between steps
            total = int(rng.integers(3, frames + 1))
            buf = torch.zeros_like(melg[r % s.B])
            n0 = int(rng.integers(0, total))
            buf[:, :n0] = melg[r % s.B][:, :n0]
            reqs[r] = dict(st=st, h=st.submit_mel(buf, uid=r, frames=n0, final=False), buf=buf, written=n0, total=total, src=r % s.B)
        else:
            n = int(rng.integers(10, s.N + 1))
            reqs[r] = dict(st=st, h=st.submit(xg[r % s.B][:, :n], uid=r))
    by_handle = {(id(q["st"]), q["h"]): r for r, q in reqs.items()}

    def take(stream, out):
        for h, (y, pcm) in out.items():
            got[by_handle[(id(stream), h)]].append((y.copy(), pcm.copy()))
        for h in stream.finished():
            finished[by_handle[(id(stream), h)]] += 1

    def produce():
        for r, q in reqs.items():
            if "buf" in q and q["written"] < q["total"] and rng.random() < 0.6:
                n = min(q["total"], q["written"] + int(rng.integers(1, 5)))
                q["buf"][:, q["written"]:n] = melg[q["src"]][:, q["written"]:n]
                q["written"] = n
                q["st"].extend_mel(q["h"], n, final=n == q["total"])

    pending = {id(st): [], id(st2): []}
    third_refused = False
    for it in range(4000):
        if not (st.busy() or st2.busy() or pending[id(st)] or pending[id(st2)]):
            break
        if it == 6:             # one running feature request moves to the second stream, with steps pending when pipelined
            r = next(r for r, q in reqs.items() if "buf" not in q and q["h"] in st.running())
            state = st.suspend(reqs[r]["h"])
            assert 0 < state.done
            reqs[r].update(st=st2, h=st2.resume(state))
            by_handle[(id(st2), reqs[r]["h"])] = r
        for stream in (st, st2):
            q = pending[id(stream)]
            if not pipelined:
                if stream.busy():
                    take(stream, stream.step(CHUNK))
                continue
            if stream.busy():
                q.append(stream.step_async(CHUNK))
            if len(stream._pending) == 2 and not third_refused:
                before = (stream.running(), stream.waiting(), list(stream._free))
                with pytest.raises(RuntimeError):
                    stream.step_async(CHUNK)
                assert before == (stream.running(), stream.waiting(), list(stream._free))
                third_refused = True
            while len(q) > (1 if stream.busy() else 0):      # two deep: step k is collected after step k + 1 has been issued
                take(stream, q.pop(0).result())
        produce()
    assert not st.busy() and not st2.busy()
    assert third_refused or not pipelined
    st.close()
    st2.close()
    return got, finished


def test_step_async_two_deep_delivers_what_step_delivers():
    a, fin_a = _service(False)
    b, fin_b = _service(True)
    assert all(v == 1 for v in fin_a.values()), fin_a
    assert all(v == 1 for v in fin_b.values()), fin_b
    for r in a:
        ya, pa = (np.concatenate([v[i] for v in a[r]]) for i in (0, 1))
        yb, pb = (np.concatenate([v[i] for v in b[r]]) for i in (0, 1))
        assert len(ya) > 0 and np.array_equal(ya, yb), "samples of request %d" % r
        assert np.array_equal(pa, pb), "PCM of request %d" % r
