"""GPU checks of endpointed decoder streams (decoder.EndpointedBeamStream / EndpointedGreedyStream) on
the planted inputs of tests/endpoint_reference.py: N = 3 streams of 70, 61 and 68 frames on a node pool of max_frames = max_segment
= 12 frames.  Under every chunking the segments are the reference's, every finished segment's beams equal the one-shot decoder on
the segment's frames alone bit for bit, the partial after every feed equals rank 0 of the one-shot decoder on the open segment's
frames, and the overflow flag stays 0.  Frames of a chunk beyond a stream's size are NaN."""
import functools
import os

import numpy as np
import pytest
import torch

import endpoint_reference as R
from beam_hot_cases import PHRASES
from test_gpu_endpoint import CHUNKINGS, DEV, N, RULE, chunk, feeds_uniform

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lm")
SENTENCES = ["THE CAT SAT ON THE MAT ", "NEW YORK IS BIG ", "THEY SAT IN THE TENT "]     # planted, one per stream (toy3's words)
TOTALS = R.TOTALS


def _bits(t):
    return t.contiguous().view(torch.int32)


def _endpointer():
    from deepspeech.pytorch_amd.decoder import Endpointer
    return Endpointer(R.THRESHOLD, *RULE)


class Case:
    """one decoder on one planted input; the one-shot oracle per slice is computed once and shared by every chunking"""

    def __init__(self, kind, B, C=29):
        from deepspeech.pytorch_amd.configs import LABELS
        from deepspeech.pytorch_amd.decoder import BeamCTCDecoder
        self.kind, self.B = kind, B
        self.labels = list(LABELS) if C == 29 else ["_", "A", "B", " ", "C"]
        assert len(self.labels) == C
        path = [[self.labels.index(ch) for ch in s] for s in SENTENCES] if C == 29 else None
        self.np = R.planted_probs(C, 11, path=path)
        self.p = torch.from_numpy(self.np).to(DEV)
        self.sil = [R.silent_mask(self.np[n, :TOTALS[n], 0], R.THRESHOLD) for n in range(N)]
        lm = os.path.join(GOLDEN, "toy3.arpa") if "lm" in kind else None
        hot = PHRASES["toy3"] if "hot" in kind else None
        self.dec = BeamCTCDecoder(self.labels, lm, 1.3, 0.7, beam_width=B, hotwords=hot)
        self._oracle = {}

    def oneshot(self, n, a, b):
        """decode_beams_detailed (ops.beam_decode / _lm / _hot / _lm_hot) on probs[n, a:b]: (strings, offsets, scores, acoustic)"""
        if (n, a, b) not in self._oracle:
            x = torch.zeros((1, max(b - a, 1), self.p.shape[2]), device=DEV)
            x[0, :b - a] = self.p[n, a:b]
            s, o, sc, ac = self.dec.decode_beams_detailed(x, torch.tensor([b - a], dtype=torch.int32))
            self._oracle[(n, a, b)] = (s[0], o[0], sc[0], ac[0])
        return self._oracle[(n, a, b)]

    def check_segment(self, n, seg, ranks):
        s, o, sc, ac = self.oneshot(n, seg.start, seg.end + 1)
        assert seg.strings == s[:ranks], (n, seg)
        assert [''.join(self.labels[v] for v in t) for t in seg.labels] == s[:ranks]
        assert len(seg.offsets) == ranks
        for r in range(ranks):
            assert seg.offsets[r].dtype == torch.int32 and torch.equal(seg.offsets[r] - seg.start, o[r]), (n, seg, r)
        assert torch.equal(_bits(seg.scores), _bits(sc[:ranks])) and torch.equal(_bits(seg.acoustic), _bits(ac[:ranks])), (n, seg)


@functools.lru_cache(maxsize=None)
def _case(kind, B, C=29):
    return Case(kind, B, C)


def _run(case, feeds, nbest, drain="every", partials=True, reset_at=None):
    """feeds `feeds`, then ends every stream; returns the drained segments per stream"""
    from deepspeech.pytorch_amd import ops
    st = case.dec.stream(N, R.MAX_SEGMENT, DEV, endpoint=_endpointer(), nbest=nbest)
    walk = [R.Walker(*RULE) for _ in range(N)]
    done, base = [0] * N, [0] * N                      # base: the frame at which the stream's numbering starts (after a reset)
    got = [[] for _ in range(N)]

    def drain_now():
        for n, segs in enumerate(st.segments()):
            got[n] += segs

    for i, s in enumerate(feeds):
        if reset_at is not None and i == reset_at:
            st.reset([1])
            walk[1], base[1], got[1] = R.Walker(*RULE), done[1], []
            assert st.frames[1] == 0
        st.feed(chunk(case.p, done, s), list(s))
        for n in range(N):
            for v in case.sil[n][done[n]:done[n] + s[n]]:
                walk[n].step(bool(v))
        done = [d + v for d, v in zip(done, s)]
        assert st.frames == [d - b for d, b in zip(done, base)]
        hdr = ops.beam_stream_header(st._h)
        assert hdr[:, 2].tolist() == [0] * N                                           # never an overflow
        assert hdr[:, 0].tolist() == [w.consumed - w.start for w in walk]              # the search holds the open segment alone
        if partials:
            text, offs = st.best()
            for n in range(N):
                a = base[n] + walk[n].start
                want = case.oneshot(n, a, done[n])
                assert text[n] == want[0][0] and torch.equal(offs[n] - walk[n].start, want[1][0]), (i, n)
        if drain == "every":
            drain_now()
    assert done == list(TOTALS)
    st.end()
    drain_now()
    assert st.segments() == [[] for _ in range(N)]
    return got, base


def _want_segments(case, n, base=0):
    return R.segments_walk(case.sil[n][base:], *RULE)


CONFIGS = [("plain", 1), ("plain", 4), ("plain", 16), ("plain", 256), ("lm", 1), ("lm", 4), ("lm", 16), ("lm", 256), ("hot", 16),
           ("lm_hot", 4)]


@pytest.mark.parametrize("name", list(CHUNKINGS))
@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: "%s-%d" % c)
def test_segments_partials_and_overflow_under_every_chunking(cfg, name):
    case = _case(*cfg)
    ranks = cfg[1] if cfg[1] in (4, 16) else 1
    feeds = CHUNKINGS[name](TOTALS)
    assert sum(TOTALS) >= 5 * N * R.MAX_SEGMENT                                         # every stream outlives max_frames five times
    got, _ = _run(case, feeds, ranks)
    for n in range(N):
        assert [(s.start, s.end, s.reason) for s in got[n]] == _want_segments(case, n), n
        assert [s.index for s in got[n]] == list(range(len(got[n])))
        for seg in got[n]:
            case.check_segment(n, seg, ranks)
    if cfg[0] == "plain":
        assert all(any(seg.strings[0] for seg in segs) for segs in got)                 # the segments are not all empty


def test_five_classes():
    case = _case("plain", 4, 5)
    got, _ = _run(case, feeds_uniform(TOTALS, 3), 4)
    for n in range(N):
        assert [(s.start, s.end, s.reason) for s in got[n]] == _want_segments(case, n)
        for seg in got[n]:
            case.check_segment(n, seg, 4)


def test_draining_once_at_the_end_gives_the_same_segments():
    """more segments end than the device ring holds: the forced fetch keeps them"""
    case = _case("plain", 4)
    every, _ = _run(case, feeds_uniform(TOTALS, 2), 4)
    once, _ = _run(case, feeds_uniform(TOTALS, 2), 4, drain="end", partials=False)
    assert [len(s) for s in once] == [8, 8, 9]
    for a, b in zip(every, once):
        assert [(s.index, s.start, s.end, s.reason, s.strings, s.labels) for s in a] == \
            [(s.index, s.start, s.end, s.reason, s.strings, s.labels) for s in b]
        for u, v in zip(a, b):
            assert all(torch.equal(x, y) for x, y in zip(u.offsets, v.offsets))
            assert torch.equal(_bits(u.scores), _bits(v.scores)) and torch.equal(_bits(u.acoustic), _bits(v.acoustic))


def test_host_chunks_in_double_precision_give_the_same_segments():
    case = _case("plain", 4)
    feeds = CHUNKINGS["uneven"](TOTALS)
    want, _ = _run(case, feeds, 4, partials=False)
    st = case.dec.stream(N, R.MAX_SEGMENT, DEV, endpoint=_endpointer(), nbest=4)
    done = [0] * N
    for s in feeds:
        st.feed(chunk(case.p, done, s).cpu().double(), list(s))
        done = [d + v for d, v in zip(done, s)]
    st.end()
    for a, b in zip(st.segments(), want):
        assert [(s.index, s.start, s.end, s.reason, s.strings) for s in a] == [(s.index, s.start, s.end, s.reason, s.strings) for s in b]
        assert all(torch.equal(_bits(u.scores), _bits(v.scores)) for u, v in zip(a, b))


@pytest.mark.parametrize("kind", ["plain", "lm"])
def test_reset_of_one_stream_in_mid_segment(kind):
    """reset([1]) after 9 feeds of 3 frames, inside stream 1's segment [20, 29]: stream 1 starts a fresh segment 0 at frame 0 on
    the frames that follow, its undrained segments are dropped; streams 0 and 2 go on as if nothing had happened"""
    case = _case(kind, 16)
    got, base = _run(case, feeds_uniform(TOTALS, 3), 16, drain="end", reset_at=9)
    assert base == [0, 27, 0]
    for n in range(N):
        want = _want_segments(case, n, base[n])
        assert [(s.start, s.end, s.reason) for s in got[n]] == want and want[0][0] == 0
        assert [s.index for s in got[n]] == list(range(len(want)))
        for seg in got[n]:
            case.check_segment(n, seg._replace(start=seg.start + base[n], end=seg.end + base[n],
                                               offsets=[o + base[n] for o in seg.offsets]), 16)


def test_greedy_segments_equal_greedy_decode_on_the_slices():
    from deepspeech.pytorch_amd.decoder import GreedyDecoder
    case = _case("plain", 4)
    dec = GreedyDecoder(case.labels)
    for name in CHUNKINGS:
        st = dec.stream(N, DEV, endpoint=_endpointer())
        done, got = [0] * N, [[] for _ in range(N)]
        whole = [''] * N
        for s in CHUNKINGS[name](TOTALS):
            added, _ = st.feed(chunk(case.p, done, s), list(s))
            done = [d + v for d, v in zip(done, s)]
            whole = [w + a for w, a in zip(whole, added)]
            assert st.frames == done
            for n, segs in enumerate(st.segments()):
                got[n] += segs
        st.end()
        for n, segs in enumerate(st.segments()):
            got[n] += segs
        for n in range(N):
            assert [(s.start, s.end, s.reason) for s in got[n]] == _want_segments(case, n), (name, n)
            for seg in got[n]:
                x = torch.zeros((1, max(seg.end + 1 - seg.start, 1), 29), device=DEV)
                x[0, :seg.end + 1 - seg.start] = case.p[n, seg.start:seg.end + 1]
                strings, offsets = dec.decode(x, torch.tensor([seg.end + 1 - seg.start], dtype=torch.int32))
                assert seg.strings == strings[0] and torch.equal(seg.offsets[0] - seg.start, offsets[0][0]), (name, n, seg)
            assert ''.join(s.strings[0] for s in got[n]) == whole[n]
        assert any(s.strings[0] for segs in got for s in segs)
    st.reset([1])
    assert st.frames[1] == 0 and st.text[1] == ''
    st.feed(case.p[:, :7], [0, 7, 0])
    assert [(s.index, s.start, s.end, s.reason) for s in st.segments()[1]] == [(0, 0, 5, "silence")]


def test_refusals_on_the_device():
    from deepspeech.pytorch_amd.decoder import BeamCTCDecoder, Endpointer
    case = _case("plain", 4)
    with pytest.raises(ValueError, match="nbest"):
        case.dec.stream(N, 12, DEV, endpoint=_endpointer(), nbest=5)
    with pytest.raises(ValueError, match="max_segment=12 passes the stream's max_frames=11"):
        case.dec.stream(N, 11, DEV, endpoint=_endpointer())
    st = case.dec.stream(N, 12, DEV, endpoint=_endpointer())
    with pytest.raises(ValueError, match="sizes"):
        st.feed(case.p[:, :4], [1, 2])
    # endpoint=None is the bounded stream that it was
    plain = case.dec.stream(N, 12, DEV)
    assert type(plain).__name__ == "BeamStream"
    with pytest.raises(ValueError, match="max_frames"):
        plain.feed(case.p[:, :13])
