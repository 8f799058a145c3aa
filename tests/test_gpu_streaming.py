"""GPU checks of streaming.StreamingTranscriber on the smallest uni-directional (LSTM + lookahead) and bi-directional GRU
fixtures: the session against the hand-written loop of the reference's run_transcribe -- model(chunk, lens, hs) per chunk, the
outputs concatenated on the time axis, one decode at the end.  The acoustic outputs come from the same calls in both arms (fp32,
eval mode), so the decoder's strings and offsets must be exactly equal; the loop also pins the carry of hs over several chunks."""
import numpy as np
import pytest
import torch

from fixtures import Fixture
from test_gpu_model import DEV, build

pytestmark = pytest.mark.gpu
CHUNKS = (17, 11, 21, 12)                        # input frames per chunk: unequal, odd and even (the fixtures have 61 and 66)


def _chunks(fx, N):
    """N clips of the fixture's batch cut into CHUNKS; with N = 2 the second stream's chunks are a little shorter"""
    inputs = fx.batch()[0]
    T = sum(CHUNKS)
    assert inputs.shape[0] >= N and inputs.shape[3] >= T
    x = torch.from_numpy(np.ascontiguousarray(inputs[:N, :, :, :T])).to(DEV)
    out, pos = [], 0
    for i, c in enumerate(CHUNKS):
        lens = [c, c - 2 * (i % 3)][:N]
        out.append((x[:, :, :, pos:pos + c].contiguous(), torch.tensor(lens, dtype=torch.int)))
        pos += c
    return out


def _loop(m, chunks):
    """the hand-written loop: per-chunk outputs (valid frames only) and the hidden state threaded through"""
    hs, outs = None, []
    with torch.no_grad():
        for x, lens in chunks:
            out, out_lens, hs = m(x, lens, hs)
            outs.append((out, out_lens))
    return outs


def _concat(outs, upto):
    """the valid frames of chunks [0, upto) back to back per stream, padded to one length, and the lengths"""
    N = outs[0][0].shape[0]
    rows = [torch.cat([o[n, :int(l[n])] for o, l in outs[:upto]]) for n in range(N)]
    sizes = torch.tensor([r.shape[0] for r in rows], dtype=torch.int)
    pad = torch.zeros((N, int(sizes.max()), rows[0].shape[1]), device=DEV)
    for n, r in enumerate(rows):
        pad[n, :r.shape[0]] = r
    return pad, sizes


@pytest.mark.parametrize("N", [1, 2])
@pytest.mark.parametrize("name", ["lstm_uni_la", "gru_bi_tiny"])
@pytest.mark.parametrize("kind", ["beam", "beam_lm", "greedy"])
def test_session_equals_the_hand_written_loop(kind, name, N):
    import os
    from deepspeech.pytorch_amd import decoder as D
    from deepspeech.pytorch_amd.streaming import StreamingTranscriber
    fx = Fixture(name)
    m = build(fx, 32).eval()
    chunks = _chunks(fx, N)
    assert len(chunks) >= 4
    outs = _loop(m, chunks)
    if kind == "greedy":
        dec = D.GreedyDecoder(fx.labels)
    elif kind == "beam":
        dec = D.BeamCTCDecoder(fx.labels, beam_width=8)
    else:
        from test_gpu_beam_lm import GOLDEN
        dec = D.BeamCTCDecoder(fx.labels, os.path.join(GOLDEN, "toy3.arpa"), 0.5, 1.0, beam_width=8, lexicon=False)
    st = StreamingTranscriber(m, dec, max_frames=sum(int(l.max()) for _, l in outs))
    assert st.best() == []
    for i, (x, lens) in enumerate(chunks):
        text = st.feed(x, lens)
        probs, sizes = _concat(outs, i + 1)
        assert st.frames == sizes.tolist()
        strings, offsets = dec.decode(probs, sizes)
        assert text == [s[0] for s in strings], (i, text)                    # the transcript after every chunk
        got = st.finish()                                                    # ... and all beams; feeding goes on afterwards
        assert got[0] == strings
        assert all(torch.equal(a, b) for u, v in zip(got[1], offsets) for a, b in zip(u, v))
    assert any(text)
    assert not m.training
    st.reset()
    assert st.hs is None and st.frames == [0] * N
    again = st.feed(*chunks[0])
    probs, sizes = _concat(outs, 1)
    assert again == [s[0] for s in dec.decode(probs, sizes)[0]]


def test_feed_wave_runs_the_front_end_per_chunk_and_training_mode_is_restored():
    from deepspeech.pytorch_amd import decoder as D
    from deepspeech.pytorch_amd.spectrogram import SpectrogramFrontEnd
    from deepspeech.pytorch_amd.streaming import StreamingTranscriber
    fx = Fixture("gru_bi_tiny")
    m = build(fx, 32).train()
    fe = SpectrogramFrontEnd(m.spect_cfg)
    dec = D.GreedyDecoder(fx.labels)
    st = StreamingTranscriber(m, dec, fe)
    rng = np.random.default_rng(1)
    wav = torch.from_numpy(rng.standard_normal((2, 3 * 4800)).astype(np.float32) * 0.1).to(DEV)
    hs, outs = None, []
    for i in range(3):
        w, ns = wav[:, i * 4800:(i + 1) * 4800].contiguous(), [4800, 4800 - 160 * i]
        text = st.feed_wave(w, ns)
        assert m.training                                                    # the session ran it in eval mode and put it back
        m.eval()
        with torch.no_grad():
            x, _, frames = fe(w, ns)
            out, out_lens, hs = m(x, frames.to(torch.int), hs)
        m.train()
        outs.append((out, out_lens))
        probs, sizes = _concat(outs, i + 1)
        assert text == [s[0] for s in dec.decode(probs, sizes)[0]] and st.frames == sizes.tolist()
    with pytest.raises(ValueError, match="streams"):
        st.feed_wave(wav[:1, :4800].contiguous(), [4800])
