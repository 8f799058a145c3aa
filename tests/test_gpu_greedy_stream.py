"""GPU checks of the streaming greedy decoder (ds2_greedy_stream_feed, ops.greedy_stream_feed, decoder.GreedyStream): greedy
output is append-only, so the labels and frames that the feeds return, concatenated, must equal ops.greedy_decode on the whole
input, under the splits of tests/test_gpu_beam_stream.py.  Frames of a chunk beyond a stream's size are NaN: they must not be read."""
import numpy as np
import pytest
import torch

from test_gpu_beam import _probs

pytestmark = pytest.mark.gpu
DEV = "cuda"
N, C = 3, 29


def _feeds_uniform(totals, chunks):
    feeds, done, i = [], [0] * len(totals), 0
    while any(d < t for d, t in zip(done, totals)):
        c = chunks[min(i, len(chunks) - 1)]
        s = tuple(min(c, t - d) for d, t in zip(done, totals))
        feeds.append(s)
        done = [d + v for d, v in zip(done, s)]
        i += 1
    return feeds


def _planted_paths(T):
    """one-hot-like rows along three paths with a repeated label (3 3 | 3) and a run of blanks (0 0 | 0 0) at frames 6 .. 9, a
    repeat separated by a blank, and the blank as the very first arg-max"""
    rng = np.random.default_rng(3)
    path = rng.integers(0, 6, size=(N, T))
    path[0, 5:9] = 3                     # boundaries at 7 and 8 fall inside the repeat
    path[1, 5:10] = 0                    # ... and inside the blank run, with the same label on both sides of it
    path[1, 4], path[1, 10] = 2, 2
    path[2, 0] = 0
    path[2, 6:9] = [4, 4, 0]
    path[2, 9] = 4
    p = np.full((N, T, C), 0.3 / (C - 1), np.float32)
    np.put_along_axis(p, path[..., None], 0.7, -1)
    return p, path


def _collapse(path, size):
    toks, offs, prev = [], [], None
    for t, c in enumerate(path[:size].tolist()):
        if c != 0 and (t == 0 or c != prev):
            toks.append(c)
            offs.append(t)
        prev = c
    return toks, offs


def _stream(p, feeds, strided=False):
    from deepspeech.pytorch_amd import ops
    n = p.shape[0]
    carry = torch.zeros((n, 2), dtype=torch.int32, device=DEV)
    toks, offs, done = [[] for _ in range(n)], [[] for _ in range(n)], [0] * n
    for s in feeds:
        w = max(max(s), 1)
        x = torch.full((w, n, C) if strided else (n, w, C), float("nan"), device=DEV)
        v = x.transpose(0, 1) if strided else x
        for i in range(n):
            v[i, :s[i]] = p[i, done[i]:done[i] + s[i]]
        t, o = ops.greedy_stream_feed(v, torch.tensor(s, dtype=torch.int32), 0, carry)
        for i in range(n):
            assert len(t[i]) == len(o[i]) <= s[i]
            toks[i] += t[i]
            offs[i] += o[i].tolist()
        done = [d + v_ for d, v_ in zip(done, s)]
        assert carry[:, 1].tolist() == done
    return toks, offs


T = 40
TOTALS = (T, T - 9, T - 2)
UNEVEN = [(5, 0, 2), (0, 9, 1), (3, 1, 35), (1, 0, 0), (0, 3, 0), (11, 0, 0), (20, 18, 0)]
SPLITS = {"one": _feeds_uniform(TOTALS, [T]), "each": _feeds_uniform(TOTALS, [1]), "7-1-15": _feeds_uniform(TOTALS, [7, 1, 15]),
          "uneven": UNEVEN}


@pytest.mark.parametrize("strided", [False, True], ids=["dense", "strided"])
@pytest.mark.parametrize("split", list(SPLITS))
@pytest.mark.parametrize("kind", ["random", "planted"])
def test_concatenated_feeds_equal_the_one_shot_decoder(kind, split, strided):
    from deepspeech.pytorch_amd import ops
    if kind == "random":
        p = _probs(np.random.default_rng(17), N, T, C)
    else:
        p, path = _planted_paths(T)
        assert (p.argmax(-1) == path).all()
        # the 7-1-15 split cuts at 7 and 8: inside stream 0's repeat, inside stream 1's blank run, after stream 2's repeat
        assert path[0, 6] == path[0, 7] == path[0, 8] == 3 and (path[1, 5:10] == 0).all() and path[1, 4] == path[1, 10] == 2
    feeds = SPLITS[split]
    assert [sum(f[i] for f in feeds) for i in range(N)] == list(TOTALS)
    dev = torch.from_numpy(p).to(DEV)
    want_t, want_o = ops.greedy_decode(dev, torch.tensor(TOTALS, dtype=torch.int32), 0)
    got_t, got_o = _stream(dev, feeds, strided)
    assert got_t == want_t and got_o == [o.tolist() for o in want_o]
    if kind == "planted":
        for i in range(N):
            assert (got_t[i], got_o[i]) == _collapse(path[i], TOTALS[i])


def test_more_than_one_wave_of_frames_in_a_chunk():
    """chunks of 64, 65 and 130 frames: the carry leaves the kernel from the lane of the chunk's last frame"""
    from deepspeech.pytorch_amd import ops
    Tl = 64 + 65 + 130 + 1
    p = _probs(np.random.default_rng(4), 2, Tl, 5, scale=1.0)     # five classes: many repeats and blanks
    dev = torch.from_numpy(p).to(DEV)
    carry = torch.zeros((2, 2), dtype=torch.int32, device=DEV)
    toks, offs, pos = [[], []], [[], []], 0
    for c in (64, 65, 130, 1):
        t, o = ops.greedy_stream_feed(dev[:, pos:pos + c], None, 0, carry)
        pos += c
        for i in range(2):
            toks[i] += t[i]
            offs[i] += o[i].tolist()
    want_t, want_o = ops.greedy_decode(dev, None, 0)
    assert toks == want_t and offs == [o.tolist() for o in want_o]


def test_greedy_stream_class_text_offsets_reset_and_host_input():
    from deepspeech.pytorch_amd.configs import LABELS
    from deepspeech.pytorch_amd.decoder import GreedyDecoder
    p = torch.from_numpy(_probs(np.random.default_rng(8), N, T, C))
    dec = GreedyDecoder(LABELS)
    st = dec.stream(N)
    pos = 0
    for c in (7, 1, 15, 17):
        strings, offs = st.feed(p[:, pos:pos + c].double() if pos else p[:, :c].to(DEV))     # a device chunk, then host chunks
        pos += c
        want, want_o = dec.decode(p[:, :pos].to(DEV))
        assert st.text == [w[0] for w in want] and st.frames == [pos] * N
        assert all(torch.equal(a, b[0]) and a.dtype == torch.int32 for a, b in zip(st.offsets, want_o))
        assert all(st.text[n].endswith(strings[n]) and len(strings[n]) == len(offs[n]) for n in range(N))
    st.reset([1])
    assert st.text[1] == '' and st.frames == [T, 0, T]
    st.feed(p[:, :9].to(DEV), [0, 9, 0])
    assert st.text[1] == dec.decode(p[1:2, :9].to(DEV))[0][0][0] and st.frames == [T, 9, T]
    with pytest.raises(ValueError, match="sizes"):
        st.feed(p[:, :4].to(DEV), [5, 0, 0])
