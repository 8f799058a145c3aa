"""GPU checks of endpointing in the sessions (StreamPool(endpoint=...), StreamingTranscriber(carry_context=True, endpoint=...);
DESIGN.md section 3.6.5) on the small uni-directional fixture model gru_uni_la with synthetic input: 2 streams of 160 and 155 input
frames, 80 and 78 output frames, on a node pool of max_frames = max_segment = 16 frames.

The rule's threshold is the median blank probability that the model itself emits for stream 0 and the counts are small, so the
fixture's own posteriors cut every stream into several segments; the reference (tests/endpoint_reference.py) says where.  The
acoustic side must not notice: the probabilities are bit-equal to a pool without endpointing."""
import functools

import numpy as np
import pytest
import torch

import endpoint_reference as R
from fixtures import DEV, Fixture
from test_gpu_model import build

pytestmark = pytest.mark.gpu
LENGTHS = [160, 155]
CHUNKS = (54, 1, 2, 37, 66)                              # the first feed is exactly the model's latency
RULE = (2, 4, 16)


def _bits(t):
    return t.contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def _setup():
    from deepspeech.pytorch_amd import synth
    fx = Fixture("gru_uni_la")
    x = torch.from_numpy(synth.synth_batch(np.asarray(LENGTHS), seed=11)[0]).to(DEV)
    return fx, build(fx, 32).eval(), x


def _decoder(fx, kind):
    from deepspeech.pytorch_amd import decoder as D
    return D.GreedyDecoder(fx.labels) if kind == "greedy" else D.BeamCTCDecoder(fx.labels, beam_width=8)


def _pool_run(pool, x, slots):
    """the lock-step schedule CHUNKS on two slots; returns (per stream the emitted probabilities per feed, the texts per feed)"""
    pos, out, texts = 0, [[], []], []
    for i, c in enumerate(CHUNKS):
        last = i == len(CHUNKS) - 1
        lens = [g - pos for g in LENGTHS] if last else [c, c]
        texts.append(pool.feed(slots, x[:, :, :, pos:pos + c].contiguous(), lens, final=slots if last else ()))
        for n, s in enumerate(slots):
            out[n].append(pool.last_output[s].clone() if s in pool.last_output else None)
        pos += c
    return out, texts


@functools.lru_cache(maxsize=None)
def _baseline():
    """a pool WITHOUT endpointing: the probabilities per feed, and from them the threshold and the reference's segments"""
    from deepspeech.pytorch_amd.decoder import Endpointer
    from deepspeech.pytorch_amd.streaming import StreamPool
    fx, m, x = _setup()
    pool = StreamPool(m, _decoder(fx, "beam"), 2, max_frames=80)
    out, _ = _pool_run(pool, x, [pool.open(), pool.open()])
    probs = [torch.cat([o for o in per if o is not None]) for per in out]
    assert [p.shape[0] for p in probs] == [80, 78]
    thr = float(np.median(probs[0][:, 0].cpu().numpy()))
    assert 0.0 < thr < 1.0
    return out, probs, Endpointer(thr, *RULE)


def _want_segments(probs, ep):
    want = [R.segments_walk(R.silent_mask(p[:, 0].cpu().numpy(), ep.blank_threshold), *RULE) for p in probs]
    assert all(len(w) >= 2 for w in want), want                                 # the fixture's own posteriors are cut
    return want


def _check_segments(dec, kind, probs, segs, want):
    assert [(s.start, s.end, s.reason) for s in segs] == want
    assert [s.index for s in segs] == list(range(len(want)))
    for s in segs:
        x = torch.zeros((1, max(s.end + 1 - s.start, 1), probs.shape[1]), device=DEV)
        x[0, :s.end + 1 - s.start] = probs[s.start:s.end + 1]
        sz = torch.tensor([s.end + 1 - s.start], dtype=torch.int32)
        if kind == "greedy":
            strings, offsets = dec.decode(x, sz)
            assert s.strings == strings[0] and torch.equal(s.offsets[0] - s.start, offsets[0][0]), s
        else:
            strings, offsets, scores, acoustic = dec.decode_beams_detailed(x, sz)
            assert s.strings == strings[0][:1] and torch.equal(s.offsets[0] - s.start, offsets[0][0]), s
            assert torch.equal(_bits(s.scores), _bits(scores[0, :1])) and torch.equal(_bits(s.acoustic), _bits(acoustic[0, :1])), s


@pytest.mark.parametrize("kind", ["beam", "greedy"])
def test_pool_segments_partials_and_untouched_probabilities(kind):
    from deepspeech.pytorch_amd.streaming import StreamPool
    fx, m, x = _setup()
    base_out, probs, ep = _baseline()
    want = _want_segments(probs, ep)
    print("threshold %.6f, segments %s" % (ep.blank_threshold, want))
    dec = _decoder(fx, kind)
    pool = StreamPool(m, dec, 2, max_frames=RULE[2], endpoint=ep)              # 80 frames on a pool of 16
    slots = [pool.open(), pool.open()]
    out, texts = _pool_run(pool, x, slots)
    emitted = [0, 0]
    for i in range(len(CHUNKS)):
        for n in range(2):
            a, b = out[n][i], base_out[n][i]
            assert (a is None) == (b is None) and (a is None or torch.equal(_bits(a), _bits(b))), (i, n)   # the acoustic side
            emitted[n] += 0 if a is None else a.shape[0]
            # the text of a feed is the partial of the open segment ('' once the final feed has closed it)
            start = max([e + 1 for _, e, r in want[n] if e < emitted[n] and r != "final"], default=0)
            if i == len(CHUNKS) - 1:
                assert texts[i][n] == ''
            elif emitted[n] > start:
                alone = dec.decode(probs[n][start:emitted[n]][None], torch.tensor([emitted[n] - start], dtype=torch.int32))
                assert texts[i][n] == alone[0][0][0], (i, n)
            else:
                assert texts[i][n] == ''
    for n, s in enumerate(slots):
        _check_segments(dec, kind, probs[n], pool.segments(s), want[n])
        assert pool.segments(s) == []
    if kind == "beam":
        from deepspeech.pytorch_amd import ops
        assert ops.beam_stream_header(pool.stream._h)[:, 2].tolist() == [0, 0]
    # slot reuse: the reopened slot has no segments and numbers its stream from frame 0, segment 0
    pool.close(slots[0])
    again = pool.open()
    assert again == slots[0] and pool.segments(again) == []
    pos, mine = 0, []
    for i, c in enumerate(CHUNKS):
        last = i == len(CHUNKS) - 1
        pool.feed([again], x[:1, :, :, pos:pos + c].contiguous(), [LENGTHS[0] - pos if last else c], final=[again] if last else ())
        if again in pool.last_output:
            mine.append(pool.last_output[again].clone())
        pos += c
    mine = torch.cat(mine)
    assert mine.shape[0] == 80
    _check_segments(dec, kind, mine, pool.segments(again), _want_segments([mine], ep)[0])


def test_pool_refuses_a_segment_that_does_not_fit_the_node_pool():
    from deepspeech.pytorch_amd.streaming import StreamPool, StreamingTranscriber
    fx, m, _ = _setup()
    _, _, ep = _baseline()
    with pytest.raises(ValueError, match="max_segment=16 passes the stream's max_frames=15"):
        StreamPool(m, _decoder(fx, "beam"), 2, max_frames=15, endpoint=ep)
    with pytest.raises(ValueError, match="max_segment=16 passes the stream's max_frames=15"):
        StreamingTranscriber(m, _decoder(fx, "beam"), max_frames=15, carry_context=True, endpoint=ep)
    with pytest.raises(ValueError, match="endpoint"):
        StreamingTranscriber(m, _decoder(fx, "beam")).segments()


@pytest.mark.parametrize("kind", ["beam", "greedy"])
def test_transcriber_segments_equal_the_decode_of_the_slices(kind):
    from deepspeech.pytorch_amd.streaming import StreamingTranscriber
    fx, m, x = _setup()
    _, _, ep = _baseline()
    dec = _decoder(fx, kind)
    st = StreamingTranscriber(m, dec, max_frames=RULE[2], carry_context=True, endpoint=ep)
    pos, out, got = 0, [[], []], [[], []]
    for i, c in enumerate(CHUNKS):
        last = i == len(CHUNKS) - 1
        text = st.feed(x[:, :, :, pos:pos + c].contiguous(), [g - pos for g in LENGTHS] if last else [c, c], final=last)
        if st.last_output is not None:
            p, sizes = st.last_output
            for n in range(2):
                out[n].append(p[n, :sizes[n]].clone())
        if i % 2 == 0:                                                           # drained now and then
            for n, segs in enumerate(st.segments()):
                got[n] += segs
        pos += c
    assert text == ['', '']
    for n, segs in enumerate(st.segments()):
        got[n] += segs
    probs = [torch.cat(o) for o in out]
    assert [p.shape[0] for p in probs] == [80, 78] and st.frames == [80, 78]
    want = _want_segments(probs, ep)
    for n in range(2):
        _check_segments(dec, kind, probs[n], got[n], want[n])


def test_pool_feed_wave():
    """raw audio: 1.6 s and 1.2 s of noise in 0.2 s feeds through the streaming front-end; the segments are the reference's on
    the probabilities that the pool emitted"""
    from deepspeech.pytorch_amd.streaming import StreamPool
    fx, m, _ = _setup()
    _, _, ep = _baseline()
    rs = np.random.RandomState(3)
    total = [25600, 19200]
    wav = [torch.from_numpy((0.1 * rs.standard_normal(n)).astype(np.float32)).to(DEV) for n in total]
    dec = _decoder(fx, "beam")
    pool = StreamPool(m, dec, 2, max_frames=RULE[2], endpoint=ep)
    slots = [pool.open(), pool.open()]
    out, pos = [[], []], 0
    while pos < total[0]:
        rows = [n for n in range(2) if pos < total[n]]
        counts = [min(3200, total[n] - pos) for n in rows]
        chunk = torch.zeros((len(rows), 3200), device=DEV)
        for r, n in enumerate(rows):
            chunk[r, :counts[r]] = wav[n][pos:pos + counts[r]]
        pool.feed_wave([slots[n] for n in rows], chunk, counts, final=[slots[n] for n in rows if pos + 3200 >= total[n]])
        for n in rows:
            if slots[n] in pool.last_output:
                out[n].append(pool.last_output[slots[n]].clone())
        pos += 3200
    probs = [torch.cat(o) for o in out]
    assert probs[0].shape[0] > 3 * RULE[2]
    want = [R.segments_walk(R.silent_mask(p[:, 0].cpu().numpy(), ep.blank_threshold), *RULE) for p in probs]
    for n in range(2):
        _check_segments(dec, "beam", probs[n], pool.segments(slots[n]), want[n])
