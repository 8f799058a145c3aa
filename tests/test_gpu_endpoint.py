"""GPU checks of the endpointing kernels alone (ds2_endpoint_*, ops.endpoint_*): after every feed the cut,
the rest, the event and the state equal the plain-Python walk of tests/endpoint_reference.py on planted inputs that hold every
edge of the rule by construction.  Frames of a chunk beyond a stream's size are NaN: they must not be read (a NaN is not silent,
so a read would break a run)."""
import ctypes

import numpy as np
import pytest
import torch

import endpoint_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
N = 3
RULE = (R.MIN_TRAILING, R.MAX_LEADING, R.MAX_SEGMENT)


def feeds_uniform(totals, c):
    feeds, done = [], [0] * len(totals)
    while any(d < t for d, t in zip(done, totals)):
        s = tuple(min(c, t - d) for d, t in zip(done, totals))
        feeds.append(s)
        done = [d + v for d, v in zip(done, s)]
    return feeds


def feeds_uneven(totals):
    """the uneven schedule of tests/test_gpu_beam_stream.py (zero sizes, stream 1 starts late), then everything that is left"""
    head = [(5, 0, 2), (0, 9, 1), (7, 1, 40), (1, 0, 0), (0, 3, 0), (11, 0, 0)]
    feeds, done = [], [0] * 3
    for f in head:
        s = tuple(min(v, t - d) for v, d, t in zip(f, done, totals))
        feeds.append(s)
        done = [d + v for d, v in zip(done, s)]
    return feeds + [tuple(t - d for d, t in zip(done, totals))]


CHUNKINGS = {"each": lambda t: feeds_uniform(t, 1), "by2": lambda t: feeds_uniform(t, 2), "by3": lambda t: feeds_uniform(t, 3),
             "uneven": feeds_uneven, "one": lambda t: feeds_uniform(t, max(t))}


def chunk(p, pos, sizes, strided=False):
    """(N, max(sizes), C) on the device: frames [pos_n, pos_n + sizes_n) of stream n, NaN beyond"""
    n, w, C = len(sizes), max(max(sizes), 1), p.shape[2]
    x = torch.full((w, n, C) if strided else (n, w, C), float("nan"), device=DEV)
    v = x.transpose(0, 1) if strided else x
    for i, (a, s) in enumerate(zip(pos, sizes)):
        v[i, :s] = p[i, a:a + s]
    return v


def run_kernel(p_host, totals, feeds, rule, threshold=R.THRESHOLD, strided=False):
    """Feeds `feeds` to ds2_endpoint_feed; a feed that stops at an endpoint goes on with the gathered rest until nothing is left.
    Every call is compared with the walk.  Returns the events per stream and facts about the feeds."""
    from deepspeech.pytorch_amd import ops
    p = torch.from_numpy(p_host).to(DEV)
    n_streams = len(totals)
    sil = [R.silent_mask(p_host[n, :totals[n], 0], threshold) for n in range(n_streams)]
    h = ops.endpoint_open(n_streams, 0, threshold, *rule, DEV)
    walk = [R.Walker(*rule) for _ in range(n_streams)]
    done = [0] * n_streams
    events = [[] for _ in range(n_streams)]
    facts = set()
    for s in feeds:
        x, take = chunk(p, done, s, strided), list(s)
        first = True
        while True:
            before = h.state.cpu()
            cut, rest, ev = ops.endpoint_feed(h, x, torch.tensor(take, dtype=torch.int32))
            want = [w.feed(sil[n][done[n]:done[n] + take[n]]) for n, w in enumerate(walk)]
            assert cut.tolist() == [c for c, _, _ in want] and rest.tolist() == [r for _, r, _ in want]
            want_ev = [[R.REASONS.index(e[0]), e[1], e[2], e[3]] if e else [0, 0, 0, 0] for _, _, e in want]
            assert ev.t().tolist() == want_ev
            after = h.state.cpu()
            assert after[:, :5].tolist() == [w.state() for w in walk] and not after[:, 5:].any()
            for n in range(n_streams):
                if take[n] == 0:
                    assert torch.equal(after[n], before[n])
                if want[n][2]:
                    events[n].append(want[n][2])
                    facts.add("last" if want[n][1] == 0 and first else "inner")
                    if want[n][0] == 1 and first:
                        facts.add("first")
            done = [d + c for d, (c, _, _) in zip(done, want)]
            take = rest.tolist()
            if not any(take):
                break
            y = ops.endpoint_gather(x, cut, rest)
            for n in range(n_streams):                                   # the frames after the cut, bit for bit
                assert torch.equal(y[n, :take[n]].view(torch.int32), p[n, done[n]:done[n] + take[n]].view(torch.int32))
            x, first = y, False
    assert done == list(totals)
    return events, facts, h


@pytest.fixture(scope="module")
def planted():
    return R.planted_probs(29, 3)


@pytest.mark.parametrize("name", list(CHUNKINGS))
def test_every_feed_equals_the_walk(name, planted):
    events, facts, _ = run_kernel(planted, R.TOTALS, CHUNKINGS[name](R.TOTALS), RULE)
    want = [R.segments_walk(R.silent_mask(planted[n, :R.TOTALS[n], 0], R.THRESHOLD), *RULE, final=False) for n in range(N)]
    assert [[(e[1], e[2], e[0]) for e in ev] for ev in events] == want             # the same segments under every chunking
    assert [e[3] for e in events[0]] == list(range(len(events[0])))
    assert {r for ev in events for r, _, _, _ in ev} == {"silence", "leading", "length"}
    if name in ("each", "by2", "by3"):
        assert {"last", "first"} <= facts              # an endpoint on the last frame of a chunk (rest 0) and on the first
    if name == "by2":
        # stream 0's run 11..13 straddles the chunk boundary 11 | 12, and its endpoint 13 is the last frame of chunk [12, 14)
        assert (0, 13, "silence") not in want[0] and (5, 13, "silence") in want[0]


def test_five_classes_and_a_strided_chunk():
    p = R.planted_probs(5, 4)
    run_kernel(p, R.TOTALS, feeds_uniform(R.TOTALS, 3), RULE)
    run_kernel(R.planted_probs(29, 5), R.TOTALS, feeds_uneven(R.TOTALS), RULE, strided=True)


def test_runs_that_straddle_the_64_frame_step():
    """one chunk of 130 frames: min_trailing = 10 silent frames 59..68 end a segment at 68, across the step boundary 63 | 64; a run
    of 9 across it does not; a run 120..129 ends a segment on the chunk's last frame; "length" falls at frame 99 in the second step"""
    sched = ("S" * 59 + "b" * 10 + "S" * 61, "S" * 58 + "b" * 9 + "S" * 53 + "b" * 10, "S" * 100)
    p = R.planted_probs(29, 6, sched)
    rule = (10, 200, 100)
    events, _, _ = run_kernel(p, (130, 130, 100), [(130, 130, 100)], rule)
    assert [(e[1], e[2], e[0]) for e in events[0]] == [(0, 68, "silence")]
    assert [(e[1], e[2], e[0]) for e in events[1]] == [(0, 99, "length"), (100, 129, "silence")]
    assert [(e[1], e[2], e[0]) for e in events[2]] == [(0, 99, "length")]
    # leading silence carried over three steps
    sched = ("b" * 150, "b" * 129 + "S" + "b" * 20, "S")
    events, _, _ = run_kernel(R.planted_probs(29, 7, sched), (150, 150, 1), [(130, 130, 1), (20, 20, 0)], (3, 140, 1000))
    assert [(e[1], e[2], e[0]) for e in events[0]] == [(0, 139, "leading")]
    assert [(e[1], e[2], e[0]) for e in events[1]] == [(0, 132, "silence")] and events[2] == []


def test_reset_and_close(planted):
    from deepspeech.pytorch_amd import ops
    _, _, h = run_kernel(planted, (20, 20, 20), feeds_uniform((20, 20, 20), 20), RULE)
    before = h.state.cpu()
    assert before[:, 3].tolist() == [20, 20, 20] and before[:, 4].tolist() == [2, 3, 2]
    ev = ops.endpoint_close(h, [0, 2]).cpu()
    after = h.state.cpu()
    assert ev.t().tolist() == [[4, 14, 19, 2], [0, 0, 0, 0], [4, 14, 19, 2]]
    assert torch.equal(after[1], before[1]) and after[[0, 2], :5].tolist() == [[20, 0, 0, 20, 3], [20, 0, 0, 20, 3]]
    assert ops.endpoint_close(h, [0]).cpu().t().tolist()[0] == [4, 20, 19, 3]        # an empty segment: end = start - 1
    ops.endpoint_reset(h, [1])
    assert h.state.cpu().tolist() == [after[0].tolist()[:4] + [4, 0, 0, 0], [0] * 8, after[2].tolist()]
    ops.endpoint_reset(h)
    assert not h.state.cpu().any()
    with pytest.raises(ValueError, match="out of range"):
        ops.endpoint_reset(h, [3])


def test_argument_errors(planted):
    from deepspeech.pytorch_amd import _lib, ops
    for kw, msg in ((dict(blank_threshold=1.5), "blank_threshold"), (dict(min_trailing=0), "min_trailing"),
                    (dict(num_streams=0), "num_streams"), (dict(device="cpu"), "HIP device"), (dict(blank=-1), "blank index")):
        good = dict(num_streams=N, blank=0, blank_threshold=0.8, min_trailing=3, max_leading=5, max_segment=12, device=DEV)
        with pytest.raises(ValueError, match=msg):
            ops.endpoint_open(**dict(good, **kw))
    h = ops.endpoint_open(N, 0, 0.8, 3, 5, 12, DEV)
    p = torch.from_numpy(planted[:, :4]).to(DEV)
    with pytest.raises(ValueError, match="shape"):
        ops.endpoint_feed(h, p[:2])
    with pytest.raises(ValueError, match="one entry per stream"):
        ops.endpoint_feed(h, p, [1, 2])
    with pytest.raises(_lib.Ds2HipError):
        ops.endpoint_feed(h, p.cpu())
    # the raw ABI: null pointers and bad counts are DS2_ERR_ARG, a misaligned state DS2_ERR_ALIGN, as for ds2_beam_stream_feed
    lib = _lib.load()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    state = torch.zeros(N * 8 + 4, dtype=torch.int32, device=DEV)
    out = torch.empty((6, N), dtype=torch.int32, device=DEV)

    def raw(Tc=4, C=29, xp=p.data_ptr(), st=state.data_ptr(), cut=out[0].data_ptr(), rest=out[1].data_ptr(), ev=out[2].data_ptr(),
            n=N, blank=0, thr=0.8, mt=3, ml=5, ms=12):
        return lib.ds2_endpoint_feed(xp, p.stride(0), p.stride(1), n, Tc, C, None, blank, thr, mt, ml, ms, st, cut, rest, ev, stream)

    assert raw() == 0
    torch.cuda.synchronize()
    assert out[0].tolist() == [4, 4, 4]
    for kw in (dict(xp=None), dict(st=None), dict(cut=None), dict(rest=None), dict(ev=None), dict(n=0), dict(Tc=0), dict(C=0),
               dict(blank=29), dict(blank=-1), dict(thr=0.0), dict(thr=1.0), dict(thr=float("nan")), dict(mt=0), dict(ml=0), dict(ms=0)):
        assert raw(**kw) == 1002, kw
    assert raw(st=state.data_ptr() + 4) == 1003
    assert lib.ds2_endpoint_reset(state.data_ptr() + 4, N, None, stream) == 1003
    assert lib.ds2_endpoint_reset(state.data_ptr(), 0, None, stream) == 1002
    assert lib.ds2_endpoint_close(state.data_ptr(), N, None, None, stream) == 1002
    assert lib.ds2_endpoint_gather(p.data_ptr(), p.stride(0), p.stride(1), N, 4, 29, out[0].data_ptr(), None, p.data_ptr(), stream) == 1002
    assert lib.ds2_endpoint_gather(p.data_ptr(), p.stride(0), p.stride(1), N, 0, 29, out[0].data_ptr(), out[1].data_ptr(), p.data_ptr(),
                                   stream) == 1002
    torch.cuda.synchronize()
