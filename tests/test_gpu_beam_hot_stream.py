"""GPU checks of the resumable beam search with hot words (ds2_beam_stream_feed_hot / _feed_lm_hot, decoder.BeamStream opened
from a BeamCTCDecoder with hotwords, and through it streaming.StreamPool).

The property is prefix equality: after any sequence of feeds that delivered frames [0, t_n) of stream n, BeamStream.result()
equals the one-shot decode_beams of the same decoder (pinned to the restatement by tests/test_gpu_beam_hot.py) on probs[n, :t_n]:
labels, frame offsets and the bits of the scores.  Frames of a chunk beyond a stream's size are NaN: they must not be read."""
import os

import numpy as np
import pytest
import torch

import beam_hot_cases as HC

pytestmark = pytest.mark.gpu
DEV = "cuda"
N, T = 3, 30
TOTALS = (T, T - 9, T - 2)


def _decoder(name, B=16, hotwords="default", **kw):
    from deepspeech.pytorch_amd.decoder import BeamCTCDecoder
    hot = HC.PHRASES[name] if hotwords == "default" else hotwords
    if name is None:
        return BeamCTCDecoder(HC.labels(), beam_width=B, hotwords=hot, **kw)
    return BeamCTCDecoder(HC.labels(), os.path.join(HC.GOLDEN, name + ".arpa"), 1.2, 0.8, beam_width=B, hotwords=hot, **kw)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    assert a[0] == b[0]
    assert all(torch.equal(x, y) for u, v in zip(a[1], b[1]) for x, y in zip(u, v))
    assert a[2].shape == b[2].shape and torch.equal(_bits(a[2]), _bits(b[2]))


def _chunk(p, pos, sizes):
    """(N, max(sizes), C): frames [pos_n, pos_n + sizes_n) of stream n, NaN beyond"""
    x = torch.full((len(sizes), max(max(sizes), 1), p.shape[2]), float("nan"), device=DEV)
    for i, (a, s) in enumerate(zip(pos, sizes)):
        x[i, :s] = p[i, a:a + s]
    return x


def _oneshot(dec, p, done):
    x = torch.zeros((len(done), max(max(done), 1), p.shape[2]), device=DEV)
    for i, t in enumerate(done):
        x[i, :t] = p[i, :t]
    return dec.decode_beams(x, torch.tensor(list(done), dtype=torch.int32))


FEEDS = {
    "one frame per feed": [tuple(int(t < total) for total in TOTALS) for t in range(T)],
    # uneven chunks; stream 1 takes nothing at first, then stream 2 and stream 0 sit out in turn
    "uneven": [(5, 0, 2), (0, 9, 1), (7, 1, 17), (1, 0, 0), (0, 3, 8), (11, 0, 0), (6, 8, 0)],
    "whole clip": [TOTALS],
}


@pytest.mark.parametrize("split", sorted(FEEDS))
@pytest.mark.parametrize("name,lexicon", [(None, False), ("toy3", True), ("toy5", False)])
def test_stream_result_equals_one_shot_decode_beams(name, lexicon, split):
    dec = _decoder(name, lexicon=lexicon)
    p = torch.from_numpy(HC.inputs(91, N, T, name)[0]).to(DEV)
    feeds = FEEDS[split]
    assert tuple(sum(f[i] for f in feeds) for i in range(N)) == TOTALS
    st = dec.stream(N, T)
    assert st._h.hot is not None and st._h.flags == (2 if name is None else 3)
    done = [0] * N
    for k, s in enumerate(feeds):
        st.feed(_chunk(p, done, s), list(s))
        done = [d + v for d, v in zip(done, s)]
        if split != "one frame per feed" or k % 7 == 3 or k + 1 == len(feeds):
            _same(st.result(), _oneshot(dec, p, done))
    assert st.frames == list(TOTALS)
    best = st.best()
    assert best[0] == [r[0] for r in st.result()[0]]


def test_reset_of_one_stream_leaves_the_others_and_an_open_stream_keeps_its_table():
    dec = _decoder("toy3", lexicon=False)
    p = torch.from_numpy(HC.inputs(92, N, T, "toy3")[0]).to(DEV)
    st = dec.stream(N, T)
    st.feed(p[:, :12])
    before = st.result()
    want = _oneshot(dec, p, [12] * N)
    _same(before, want)
    dec.set_hotwords([("TENT", 1.0)])                      # for calls and streams from now on: the open stream keeps its table
    st.reset([1])
    after = st.result()
    for n in (0, 2):
        assert after[0][n] == before[0][n] and torch.equal(_bits(after[2][n]), _bits(before[2][n]))
    assert after[0][1][0] == '' and float(after[2][1, 0]) == 0.0 and st.frames == [12, 0, 12]
    st.feed(_chunk(p, [12, 0, 12], (5, 12, 0)), [5, 12, 0])
    got = st.result()
    dec.set_hotwords(HC.PHRASES["toy3"])
    _same(got, _oneshot(dec, p, [17, 12, 12]))
    # a stream opened while other phrases were set differs
    dec.set_hotwords([("TENT", 1.0)])
    other = dec.stream(N, T)
    other.feed(p[:, :12])
    _same(other.result(), _oneshot(dec, p, [12] * N))
    assert not torch.equal(_bits(other.result()[2]), _bits(want[2]))


def test_stream_pool_with_two_staggered_slots_gives_the_one_shot_partials():
    """the pool's transcript after every feed is the decoder's one-shot decode, hot words included, of the frames emitted so far"""
    from deepspeech.pytorch_amd import decoder as D
    from deepspeech.pytorch_amd.streaming import StreamPool
    from fixtures import Fixture
    from test_gpu_model import build
    fx = Fixture("lstm_uni_la")
    x = torch.from_numpy(np.ascontiguousarray(fx.batch()[0])).to(DEV)
    lengths = [int(v) for v in fx.z["input_sizes"]]
    m = build(fx, 32).eval()
    plain = D.BeamCTCDecoder(fx.labels, beam_width=8)
    with torch.no_grad():
        probs, sizes = m(x, torch.tensor(lengths, dtype=torch.int))[:2]
    words = [w for s in plain.decode(probs, sizes)[0] for w in s[0].split(' ') if w]
    letters = [c for c in fx.labels[1:] if c != ' '][:3]
    hot = sorted(set(words[:2] + letters))                 # whole words of the plain transcripts, and single letters
    dec = D.BeamCTCDecoder(fx.labels, beam_width=8, hotwords=[(w, 1.5) for w in hot])
    assert not torch.equal(dec.decode_beams(probs, sizes)[2], plain.decode_beams(probs, sizes)[2])        # the boost is in use
    pool = StreamPool(m, dec, 2)
    starts, chunks = (0, 1), (17, 11, 21, 9)
    slot, fed, nfeeds, done, got = {}, [0, 0], [0, 0], [False, False], [[], []]
    tick = checked = 0
    while not all(done):
        for k in range(2):
            if starts[k] == tick:
                slot[k] = pool.open()
        rows = [k for k in range(2) if k in slot and not done[k]]
        lens = [min(chunks[nfeeds[k] % len(chunks)], lengths[k] - fed[k]) for k in rows]
        final = [k for k, c in zip(rows, lens) if fed[k] + c == lengths[k]]
        xc = torch.zeros((len(rows), 1, x.shape[2], max(lens)), device=DEV)
        for r, k in enumerate(rows):
            xc[r, :, :, :lens[r]] = x[k, :, :, fed[k]:fed[k] + lens[r]]
        texts = pool.feed([slot[k] for k in rows], xc, lens, final=[slot[k] for k in final])
        for r, k in enumerate(rows):
            out = pool.last_output.get(slot[k])
            if out is not None:
                got[k].append(out.clone())
            fed[k] += lens[r]
            nfeeds[k] += 1
            done[k] = k in final
            if got[k]:
                q = torch.cat(got[k])[None]
                alone = dec.decode(q, torch.tensor([q.shape[1]], dtype=torch.int))[0][0][0]
                assert texts[r] == alone, (tick, k)
                checked += 1
        tick += 1
    assert checked >= 4 and pool.stream._h.hot is not None
