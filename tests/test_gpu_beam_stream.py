"""GPU checks of the resumable beam search (ds2_beam_stream_*, ops.beam_stream_*, decoder.BeamStream).

The property is prefix equality: after any sequence of feeds that delivered frames [0, t_n) of stream n, the stream's result
equals the one-shot decoder (ops.beam_decode / ops.beam_decode_lm, pinned to the host restatements by tests/test_gpu_beam.py and
tests/test_gpu_beam_lm.py) on probs[n, :t_n] on the same device: labels, frame offsets, lengths, scores and acoustic scores, bit for
bit.  It is checked after every feed of every split.  Frames of a chunk beyond a stream's size are NaN: they must not be read."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from beam_lm_reference import Scorer, beam_search_lm
from beam_reference import beam_search
from test_gpu_beam import _check as _check_plain, _probs
from test_gpu_beam_lm import DEV, SENTENCES, _check as _check_lm, _inputs, _labels, _lm, _planted, _tables

pytestmark = pytest.mark.gpu
N = 3


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    """two results of beam_decode (3 values) or beam_decode_lm (4): labels, offsets and the bits of the scores"""
    assert len(a) == len(b)
    assert a[0] == b[0]
    assert all(torch.equal(x, y) for u, v in zip(a[1], b[1]) for x, y in zip(u, v))
    for x, y in zip(a[2:], b[2:]):
        assert x.shape == y.shape and torch.equal(_bits(x), _bits(y))


class Case:
    """one decoder configuration on one input: the one-shot oracle per prefix (computed once per prefix and shared)"""

    def __init__(self, p, B, top_n=40, cutoff_prob=1.0, lm=None, lexicon=True, alpha=1.3, beta=0.7):
        self.p = torch.from_numpy(p).to(DEV)
        self.np = p
        self.C = p.shape[2]
        self.B, self.top_n, self.cutoff_prob, self.lm_name, self.lexicon, self.alpha, self.beta = B, top_n, cutoff_prob, lm, lexicon, alpha, beta
        self._oracle = {}

    def lm_args(self):
        if self.lm_name is None:
            return None
        wt, gt = _tables(self.lm_name)
        m = _lm(self.lm_name)
        return dict(space=_labels().index(' '), word_table=wt, ngram_table=gt, order=m.order, bos=m.bos, alpha=self.alpha,
                    beta=self.beta, lexicon=self.lexicon)

    def open(self, max_frames, streams=N):
        from deepspeech.pytorch_amd import ops
        return ops.beam_stream_open(streams, max_frames, self.C, 0, self.B, self.top_n, self.cutoff_prob, DEV, self.lm_args())

    def oneshot(self, t, start=None):
        """the one-shot decoder on frames [start_n, start_n + t_n) of every stream"""
        from deepspeech.pytorch_amd import ops
        start = tuple(start) if start is not None else (0,) * len(t)
        key = (tuple(t), start)
        if key not in self._oracle:
            x = self.chunk(start, t, nan=False)
            sz = torch.tensor(list(t), dtype=torch.int32)
            if self.lm_name is None:
                r = ops.beam_decode(x, sz, 0, self.B, self.top_n, self.cutoff_prob)
            else:
                L = self.lm_args()
                r = ops.beam_decode_lm(x, sz, 0, self.B, self.top_n, self.cutoff_prob, L["space"], L["word_table"], L["ngram_table"],
                                       L["order"], L["bos"], L["alpha"], L["beta"], L["lexicon"])
            self._oracle[key] = r
        return self._oracle[key]

    def chunk(self, pos, sizes, nan=True, strided=False):
        """(N, max(sizes), C): frames [pos_n, pos_n + sizes_n) of stream n, NaN beyond"""
        n, w = len(sizes), max(max(sizes), 1)
        x = torch.full((w, n, self.C) if strided else (n, w, self.C), float("nan") if nan else 0.0, device=DEV)
        v = x.transpose(0, 1) if strided else x
        for i, (a, s) in enumerate(zip(pos, sizes)):
            v[i, :s] = self.p[i, a:a + s]
        return v


def _feeds_uniform(totals, chunks):
    """per-feed sizes for chunk lengths `chunks` (the last repeated): every stream takes what it has left of the chunk"""
    feeds, done = [], [0] * len(totals)
    i = 0
    while any(d < t for d, t in zip(done, totals)):
        c = chunks[min(i, len(chunks) - 1)]
        s = [min(c, t - d) for d, t in zip(done, totals)]
        feeds.append(tuple(s))
        done = [d + v for d, v in zip(done, s)]
        i += 1
    return feeds


def _feeds_uneven(totals):
    """the streams advance unevenly: stream 1 gets nothing in the first feed, stream 2 finishes early, zeros in between"""
    head = [(5, 0, 2), (0, 9, 1), (7, 1, 40), (1, 0, 0), (0, 3, 0), (11, 0, 0)]
    feeds, done = [], [0] * 3
    for f in head:
        s = tuple(min(v, t - d) for v, d, t in zip(f, done, totals))
        feeds.append(s)
        done = [d + v for d, v in zip(done, s)]
    assert done[2] == totals[2] and done[0] < totals[0]               # stream 2 has finished, the others have not
    return feeds + [tuple(t - d for d, t in zip(done, totals))]


def _run(case, feeds, totals, strided=False, check=True):
    """feeds the sizes of `feeds`, after every feed the result against the one-shot decoder on the prefix; returns the handle"""
    from deepspeech.pytorch_amd import ops
    h = case.open(max(totals))
    done = [0] * len(totals)
    for s in feeds:
        x = case.chunk(done, s, strided=strided)
        assert ops.beam_stream_feed(h, x, torch.tensor(s, dtype=torch.int32)) is None
        done = [d + v for d, v in zip(done, s)]
        if check:
            _same(ops.beam_stream_result(h, max(done)), case.oneshot(done))
    assert done == list(totals)
    hdr = ops.beam_stream_header(h)
    assert hdr[:, 0].tolist() == list(totals) and hdr[:, 2].tolist() == [0] * len(totals)
    return h


T = 40
TOTALS = (T, T - 9, T - 2)


@functools.lru_cache(maxsize=None)
def _plain_case(C, B, top_n, cutoff_prob):
    return Case(_probs(np.random.default_rng(100 + C), N, T, C), B, top_n, cutoff_prob)


@functools.lru_cache(maxsize=None)
def _lm_case(name, B, lexicon, cutoff_prob):
    return Case(_inputs(7 + B, N, T, name)[0], B, 40, cutoff_prob, name, lexicon)


PLAIN = [(29, 1, 40, 1.0), (29, 4, 40, 1.0), (29, 16, 40, 1.0), (29, 256, 40, 1.0), (29, 16, 5, 1.0), (29, 16, 40, 0.9), (29, 4, 5, 0.9),
         (6, 4, 40, 1.0), (6, 16, 40, 1.0), (6, 256, 5, 0.9)]
LM = [("toy3", 16, True, 1.0), ("toy3", 256, False, 1.0), ("toy5", 4, True, 1.0), ("toy1", 1, False, 1.0), ("toy5", 16, False, 0.9),
      ("toy1", 256, True, 0.9)]
SPLITS = {"one": lambda: _feeds_uniform(TOTALS, [T]), "each": lambda: _feeds_uniform(TOTALS, [1]),
          "7-1-15": lambda: _feeds_uniform(TOTALS, [7, 1, 15]), "uneven": lambda: _feeds_uneven(TOTALS)}


@pytest.mark.parametrize("split", list(SPLITS))
@pytest.mark.parametrize("cfg", PLAIN, ids=lambda c: "-".join(str(v) for v in c))
def test_every_prefix_equals_the_one_shot_decoder(cfg, split):
    """B = 256 and 16 meet the first boundaries while nb < B (one frame gives at most C candidates per beam)"""
    _run(_plain_case(*cfg), SPLITS[split](), TOTALS)


@pytest.mark.parametrize("split", list(SPLITS))
@pytest.mark.parametrize("cfg", LM, ids=lambda c: "-".join(str(v) for v in c))
def test_every_prefix_equals_the_one_shot_decoder_with_lm(cfg, split):
    _run(_lm_case(*cfg), SPLITS[split](), TOTALS)


def test_final_results_pass_the_host_restatements():
    """one case without and one with an LM: the streamed final result under the acceptance rule of the existing beam tests"""
    from deepspeech.pytorch_amd import ops
    case = _plain_case(29, 16, 40, 1.0)
    toks, offs, scores = ops.beam_stream_result(_run(case, _feeds_uniform(TOTALS, [7, 1, 15]), TOTALS, check=False))
    _check_plain(toks, offs, scores, case.np, np.array(TOTALS, np.int32), 0, 16, 40, 1.0)
    case = _lm_case("toy3", 16, True, 1.0)
    toks, offs, scores, acoustic = ops.beam_stream_result(_run(case, _feeds_uneven(TOTALS), TOTALS, check=False))
    sc = Scorer(_lm("toy3"), _labels(), 0, case.alpha, case.beta, True, np.float32)
    refs = [beam_search_lm(case.np[n], TOTALS[n], 0, 16, 40, 1.0, sc) for n in range(N)]
    assert sum(r["word_events"] for r in refs) >= 1
    _check_lm(toks, offs, scores, acoustic, refs, 16)


@functools.lru_cache(maxsize=None)
def _planted_case(lexicon):
    """clean planted sentences (little noise: the arg-max path is the planted path), and per stream a boundary of each kind"""
    labels = _labels()
    rng = np.random.default_rng(5)
    p = np.stack([_planted(rng, T, SENTENCES["toy3"], labels, peak=6.0, noise=0.5) for _ in range(N)])
    path = p.argmax(-1)
    sp = labels.index(' ')
    kinds = {"repeat": lambda a, b: a == b and a not in (0, sp), "after_space": lambda a, b: a == sp and b != sp,
             "mid_word": lambda a, b: a != b and a not in (0, sp) and b not in (0, sp)}
    cuts = {k: [next(t for t in range(2, int(0.8 * T)) if f(path[n, t - 1], path[n, t])) for n in range(N)] for k, f in kinds.items()}
    return Case(p, 16, 40, 1.0, "toy3", lexicon), cuts


@pytest.mark.parametrize("lexicon", [True, False], ids=["lexicon", "open"])
@pytest.mark.parametrize("kind", ["repeat", "after_space", "mid_word"])
def test_boundaries_planted_inside_repeats_after_spaces_and_inside_words(kind, lexicon):
    """the first feed ends, per stream, between two frames of one repeated label / right after a space / inside a word"""
    case, cuts = _planted_case(lexicon)
    cut = cuts[kind]
    totals = (T, T, T)
    _run(case, [tuple(cut), tuple(T - c for c in cut)], totals)
    _run(case, [tuple(c - 1 for c in cut), (1, 1, 1), (1, 1, 1), tuple(T - c - 1 for c in cut)], totals)


def test_boundary_before_a_merge_through_an_old_node():
    """A prefix that was pruned and re-created merges with children that hang off its old node (tests/test_gpu_beam.py's input,
    the three utterances with most such merges); the feed boundary is put directly before the frame of the first such merge, so
    that the merge in the next chunk goes through a node, a hash and a frame that came in with the stored state."""
    p = _probs(np.random.default_rng(33), 64, 40, 3, scale=1.0)
    count = lambda n, t: beam_search(p[n], t, 0, 3, 40, 1.0)["revival_merges"]
    pick = sorted(range(64), key=lambda n: -count(n, 40))[:N]
    assert all(count(n, 40) > 0 for n in pick)
    cut = [next(t for t in range(1, 41) if count(n, t) > 0) - 1 for n in pick]     # the merge happens in frame cut[n]
    assert all(c >= 1 for c in cut)
    case = Case(np.ascontiguousarray(p[pick]), 3)
    _run(case, [tuple(cut), (1, 1, 1), tuple(40 - c - 1 for c in cut)], (40, 40, 40))
    _run(case, _feeds_uniform((40, 40, 40), [1]), (40, 40, 40))


def test_strided_chunks():
    for case in (_plain_case(29, 16, 40, 1.0), _lm_case("toy3", 16, True, 1.0)):
        _run(case, _feeds_uniform(TOTALS, [7, 1, 15]), TOTALS, strided=True)


def _decoder(case):
    import os
    from deepspeech.pytorch_amd.decoder import BeamCTCDecoder
    from test_gpu_beam_lm import GOLDEN
    if case.lm_name is None:
        return BeamCTCDecoder(_labels(), beam_width=case.B, cutoff_top_n=case.top_n, cutoff_prob=case.cutoff_prob)
    return BeamCTCDecoder(_labels(), os.path.join(GOLDEN, case.lm_name + ".arpa"), case.alpha, case.beta, case.top_n, case.cutoff_prob,
                          case.B, lexicon=case.lexicon)


@pytest.mark.parametrize("lm", [False, True], ids=["plain", "lm"])
def test_beam_stream_host_input_result_twice_best_and_frames(lm):
    """decoder.BeamStream on host tensors: result() twice gives the same and does not disturb later feeds; best() is rank 0"""
    case = _lm_case("toy3", 16, True, 1.0) if lm else _plain_case(29, 16, 40, 1.0)
    dec = _decoder(case)
    st = dec.stream(N, T)
    done = [0] * N
    for s in _feeds_uneven(TOTALS):
        st.feed(case.chunk(done, s).cpu().double(), list(s))                # a host tensor, fp64, host ints
        done = [d + v for d, v in zip(done, s)]
        assert st.frames == done
        a, b = st.result(), st.result()
        assert a[0] == b[0] and torch.equal(_bits(a[2]), _bits(b[2]))
        assert all(torch.equal(x, y) for u, v in zip(a[1], b[1]) for x, y in zip(u, v))
        want = dec.decode_beams(case.chunk([0] * N, done, nan=False), torch.tensor(done))
        assert a[0] == want[0] and torch.equal(_bits(a[2]), _bits(want[2]))
        assert all(torch.equal(x, y) and x.dtype == torch.int32 for u, v in zip(a[1], want[1]) for x, y in zip(u, v))
        best = st.best()
        assert best[0] == [s_[0] for s_ in a[0]] and all(torch.equal(x, y[0]) for x, y in zip(best[1], a[1]))
    assert done == list(TOTALS)
    st.reset()
    assert st.frames == [0] * N and st.result()[0] == [[''] * 16] * N


@pytest.mark.parametrize("lm", [False, True], ids=["plain", "lm"])
def test_reset_of_one_stream_in_mid_stream(lm):
    """after reset([1]) stream 1 equals a fresh decode of what follows; streams 0 and 2 equal their uninterrupted decode"""
    from deepspeech.pytorch_amd import ops
    case = _lm_case("toy3", 16, False, 1.0) if lm else _plain_case(6, 16, 40, 1.0)
    h = case.open(T)
    first, rest = (13, 13, 13), (T - 13, T - 13, T - 13)
    ops.beam_stream_feed(h, case.chunk((0, 0, 0), first), None)
    ops.beam_stream_reset(h, [1])
    assert ops.beam_stream_header(h)[:, 0].tolist() == [13, 0, 13]
    mid = ops.beam_stream_result(h, 13)
    pick = lambda res: [[r[0], r[2]] if isinstance(r, list) else r[[0, 2]] for r in res]
    _same(pick(mid), pick(case.oneshot(first)))
    assert mid[0][1] == [[]] * 16 and mid[2][1].tolist() == [0.0] + [float("inf")] * 15
    ops.beam_stream_feed(h, case.chunk(first, rest), None)
    got = ops.beam_stream_result(h, T)
    whole, tail = case.oneshot((T, T, T)), case.oneshot(rest, start=first)
    for n, ref in ((0, whole), (1, tail), (2, whole)):
        assert got[0][n] == ref[0][n]
        assert all(torch.equal(x, y) for x, y in zip(got[1][n], ref[1][n]))  # stream 1's frames count from its reset
        for x, y in zip(got[2:], ref[2:]):
            assert torch.equal(_bits(x[n]), _bits(y[n]))


def test_capacity():
    from deepspeech.pytorch_amd import ops
    from deepspeech.pytorch_amd.decoder import BeamCTCDecoder
    case = _plain_case(29, 16, 40, 1.0)
    # max_frames exactly reached is fine; one frame more raises before anything is launched and leaves the state as it was
    st = BeamCTCDecoder(_labels(), beam_width=16).stream(N, 12)
    st.feed(case.p[:, :5])
    st.feed(case.p[:, 5:12], [7, 7, 6])
    before = st.result()
    with pytest.raises(ValueError, match="max_frames"):
        st.feed(case.p[:, 12:14], [0, 0, 2])
    assert st.frames == [12, 12, 11] and ops.beam_stream_header(st._h)[:, [0, 2]].tolist() == [[12, 0], [12, 0], [11, 0]]
    _same(st.result(), before)
    st.feed(case.p[:, 11:12], [0, 0, 1])
    assert st.frames == [12, 12, 12]
    assert st.result()[0] == BeamCTCDecoder(_labels(), beam_width=16).decode_beams(case.p[:, :12])[0]
    # the ops-level entry: the kernel consumes nothing for the stream that would pass max_frames and raises its flag
    h = case.open(4)
    ops.beam_stream_feed(h, case.p[:, :3], torch.tensor([3, 1, 0], dtype=torch.int32))
    ops.beam_stream_feed(h, case.p[:, 3:9], torch.tensor([6, 3, 4], dtype=torch.int32))         # stream 0: 3 + 6 > 4
    assert ops.beam_stream_header(h)[:, [0, 2]].tolist() == [[3, 1], [4, 0], [4, 0]]
    got = ops.beam_stream_result(h, 4)
    x = torch.stack([case.p[0, :4], torch.cat([case.p[1, :1], case.p[1, 3:6]]), case.p[2, 3:7]])
    _same(got, ops.beam_decode(x, torch.tensor([3, 4, 4], dtype=torch.int32), 0, 16, 40, 1.0))


def test_argument_errors():
    """the messages of the one-shot wrappers, and the raw ABI's refusals"""
    from deepspeech.pytorch_amd import _lib, ops
    case = _lm_case("toy3", 16, True, 1.0)
    L = case.lm_args()
    C = case.C
    for kw, msg in ((dict(beam_width=257), "beam_width must be in"), (dict(beam_width=0), "beam_width must be in"),
                    (dict(cutoff_top_n=0), "cutoff_top_n"), (dict(blank=C), "blank index"), (dict(num_classes=8193), "up to 8192 classes"),
                    (dict(lm=dict(L, space=0)), "space label"), (dict(lm=dict(L, order=6)), "language-model order"),
                    (dict(lm=dict(L, bos=-1)), "id of <s>"), (dict(lm=dict(L, word_table=L["word_table"][:3])), "power of two"),
                    (dict(lm=dict(L, ngram_table=L["ngram_table"].cpu())), "must live on the device"),
                    (dict(num_streams=0), "num_streams"), (dict(max_frames=0), "max_frames")):
        good = dict(num_streams=N, max_frames=8, num_classes=C, blank=0, beam_width=4, cutoff_top_n=40, cutoff_prob=1.0, device=DEV)
        with pytest.raises(ValueError, match=msg):
            ops.beam_stream_open(**dict(good, **kw))
    h = case.open(8)
    with pytest.raises(ValueError, match="shape"):
        ops.beam_stream_feed(h, case.p[:2, :4])
    with pytest.raises(ValueError, match="one entry per stream"):
        ops.beam_stream_feed(h, case.p[:, :4], [1, 2])
    with pytest.raises(ValueError, match="out of range"):
        ops.beam_stream_reset(h, [3])
    with pytest.raises(_lib.Ds2HipError):
        ops.beam_stream_feed(h, case.p[:, :4].cpu())
    # the raw ABI
    lib = _lib.load()
    B, F = 4, 8
    state = torch.empty(lib.ds2_beam_stream_bytes(N, B, F, 0), dtype=torch.uint8, device=DEV)
    ws = torch.empty(lib.ds2_beam_stream_ws_bytes(N, 4), dtype=torch.uint8, device=DEV)
    buf = torch.empty((2, N, B, F), dtype=torch.int32, device=DEV)
    lens = torch.empty((N, B), dtype=torch.int32, device=DEV)
    scores = torch.empty((N, B), dtype=torch.float32, device=DEV)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    x = case.p[:, :4].contiguous()
    assert lib.ds2_beam_stream_reset(state.data_ptr(), N, B, F, 0, None, stream) == 0

    def raw(Tc=4, xp=x.data_ptr(), st=state.data_ptr(), tok=buf[0].data_ptr(), off=buf[1].data_ptr(), ln=lens.data_ptr(),
            sc=scores.data_ptr(), w=ws.data_ptr(), B=B, F=F, top_n=40, R=None):
        return lib.ds2_beam_stream_feed(xp, x.stride(0), x.stride(1), N, Tc, C, None, 0, B, top_n, 1.0, st, F, tok, off, F,
                                        B if R is None else R, ln, sc, w, stream)

    assert raw() == 0 and raw(tok=None, off=None, ln=None, sc=None) == 0 and raw(Tc=0, xp=None, w=None) == 0
    torch.cuda.synchronize()
    for kw in (dict(st=None), dict(off=None), dict(sc=None), dict(xp=None), dict(w=None), dict(B=257), dict(B=0), dict(F=0),
               dict(top_n=0), dict(Tc=-1), dict(R=0), dict(R=5), dict(Tc=0, tok=None, off=None, ln=None, sc=None)):
        assert raw(**kw) == 1002, kw                                          # DS2_ERR_ARG
    assert raw(st=state.data_ptr() + 16) == 1003                              # DS2_ERR_ALIGN
    assert lib.ds2_beam_stream_reset(None, N, B, F, 0, None, stream) == 1002
    torch.cuda.synchronize()
