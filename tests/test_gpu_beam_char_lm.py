"""GPU checks of the device beam search with a character n-gram language model (ds2_beam_decode_clm and its stream and grid
forms, ops.beam_decode_clm, decoder.BeamCTCDecoder with lm_unit="char") against the numpy restatement of its rules
(tests/beam_char_lm_reference.py, itself pinned by tests/test_beam_char_lm_reference.py).  The comparison is that of
tests/test_gpu_beam_lm.py: the same set of strings with exact frames, totals and acoustic scores within 1e-4 relative, and the
order by rank except where adjacent totals lie within 1e-6 relative.

test_skipped_ranks_stay_under_the_cap counts the ranks that this last rule leaves uncompared by position: rank 0 of every
utterance with frames is compared, and at most 5 % of all ranks of the grid are skipped.  Counted with the restatement on the
CPU for the inputs below: 8 of 1 601 ranks skipped (0.5 %), never rank 0."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from beam_char_lm_reference import CharScorer, beam_search_clm
from beam_reference import beam_search
from test_gpu_beam_lm import SENTENCES, _check, _near, _planted, _softmax

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lm")
FILES = {1: "char1", 3: "char3", 5: "char5", "cjk": "cjk3"}
CJK_LABELS = ["_"] + [chr(0x4E00 + i) for i in range(300)]


def _labels(cjk=False):
    from deepspeech.pytorch_amd.configs import LABELS
    return CJK_LABELS if cjk else list(LABELS)


def _path(name):
    return os.path.join(GOLDEN, name + ".arpa")


@functools.lru_cache(maxsize=None)
def _lm(name):
    from deepspeech.pytorch_amd import lm
    return lm.load_arpa(_path(name))


@functools.lru_cache(maxsize=None)
def _tables(name, space_token):
    from deepspeech.pytorch_amd import lm
    ids, gt = lm.build_char_tables(_lm(name), _labels(name == "cjk3"), 0, space_token)
    return torch.from_numpy(ids).to(DEV), torch.from_numpy(gt).to(DEV)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    """two results of beam_decode (3 values) or beam_decode_clm (4): labels, offsets and the bits of the scores"""
    assert len(a) == len(b)
    assert a[0] == b[0]
    assert all(torch.equal(x, y) for u, v in zip(a[1], b[1]) for x, y in zip(u, v))
    for x, y in zip(a[2:], b[2:]):
        assert x.shape == y.shape and torch.equal(_bits(x), _bits(y))


def _planted_cjk(rng, T):
    """(T, 301) probabilities: a walk over the stored bigrams of cjk3.arpa, one or two frames a label, as peaky rows with noise"""
    m = _lm("cjk3")
    nxt = {}
    for a, b in m.ids[1].tolist():
        if a >= 3 and b >= 3:
            nxt.setdefault(a, []).append(b)
    cur, path = sorted(nxt)[int(rng.integers(0, len(nxt)))], []
    while len(path) < T:
        c = CJK_LABELS.index(m.words[cur])
        if path and (path[-1] == c or rng.random() < 0.3):
            path.append(0)
        path += [c] * int(rng.integers(1, 3))
        cur = nxt[cur][int(rng.integers(0, len(nxt[cur])))] if cur in nxt else sorted(nxt)[int(rng.integers(0, len(nxt)))]
    z = rng.standard_normal((T, len(CJK_LABELS))) * 1.5
    z[np.arange(T), path[:T]] += 6.0
    return _softmax(z)


def _inputs(seed, N, T, cjk=False):
    rng = np.random.default_rng(seed)
    labels = _labels()
    if cjk:
        p = np.stack([_planted_cjk(rng, T) for _ in range(N)])
    else:
        p = np.stack([_planted(rng, T, SENTENCES["toy3"] if T > 2 else ["A"], labels) for _ in range(N)])
    sizes = rng.integers(1, T + 1, size=N)
    sizes[0] = T
    if N >= 3:
        sizes[1] = 0
    return p, sizes.astype(np.int32)


# (N, T, B, order or "cjk", space_token, cutoff_prob, strided (T, N, C) view, cutoff_top_n, alpha, beta)
GRID = [
    (1, 2, 256, 3, None, 1.0, False, 40, 1.2, 0.8),
    (1, 17, 256, 3, "|", 1.0, False, 40, 1.0, 1.0),
    (3, 17, 10, 5, "|", 1.0, True, 40, 1.3, 0.7),
    (3, 17, 128, 1, "|", 0.9, False, 40, 0.5, 2.0),
    (3, 2, 1, 3, "|", 1.0, False, 40, 1.0, 1.0),
    (8, 17, 1, 1, None, 1.0, False, 40, 2.0, 0.0),
    (2, 61, 16, 3, "|", 1.0, False, 40, 0.9, 1.1),
    (2, 61, 256, 5, "|", 0.9, False, 40, 1.1, 0.3),
    (1, 200, 128, 3, "|", 1.0, False, 40, 0.8, 1.5),
    (2, 40, 64, "cjk", None, 1.0, False, 64, 1.0, 0.5),
]


@functools.lru_cache(maxsize=None)
def _case(N, T, B, order, space_token, cutoff_prob, strided, top_n, alpha, beta):
    """the case's inputs and the restatement's result per utterance (made once, on the CPU)"""
    cjk = order == "cjk"
    p, sizes = _inputs(N * 1000 + T * 7 + B, N, T, cjk)
    sc = CharScorer(_lm(FILES[order]), _labels(cjk), 0, alpha, beta, space_token, np.float32)
    refs = [beam_search_clm(p[n], sizes[n], 0, B, top_n, cutoff_prob, sc) for n in range(N)]
    return p, sizes, refs


@pytest.mark.parametrize("case", GRID, ids=lambda c: "-".join(str(v) for v in c))
def test_kernel_matches_restatement(case):
    from deepspeech.pytorch_amd import ops
    N, T, B, order, space_token, cutoff_prob, strided, top_n, alpha, beta = case
    p, sizes, refs = _case(*case)
    assert sum(r["label_events"] for r in refs) >= 1
    if strided:
        view = torch.from_numpy(np.ascontiguousarray(p.transpose(1, 0, 2))).to(DEV).transpose(0, 1)
        assert not view.is_contiguous()
    else:
        view = torch.from_numpy(p).to(DEV)
    name = FILES[order]
    ids, gt = _tables(name, space_token)
    if order == "cjk":
        assert min(top_n, p.shape[2]) == 64 and int(ids.max()) > 255
    m = _lm(name)
    toks, offs, scores, acoustic = ops.beam_decode_clm(view, torch.from_numpy(sizes), 0, B, top_n, cutoff_prob, ids, gt, m.order,
                                                       m.bos, alpha, beta)
    assert scores.shape == (N, B) and acoustic.shape == (N, B) and len(toks) == N and all(len(t) == B for t in toks)
    _check(toks, offs, scores, acoustic, refs, B)


def test_skipped_ranks_stay_under_the_cap():
    """the 1e-6 rule of the rank comparison: rank 0 of every utterance with frames is compared by position, and no more than 5 %
    of all ranks of the grid are skipped (8 of 1 601 with these inputs)"""
    skipped = total = oov = 0
    for case in GRID:
        _, sizes, refs = _case(*case)
        oov += sum(r["oov_events"] for r in refs)
        for n, ref in enumerate(refs):
            rb = ref["beams"]
            total += len(rb)
            skipped += sum(_near(rb, b) for b in range(len(rb)))
            if sizes[n] > 0:
                assert not _near(rb, 0), (case, n)
    print("skipped ranks: %d of %d" % (skipped, total))
    assert total > 1000 and skipped <= 0.05 * total, (skipped, total)
    assert oov > 100                                             # labels that the files do not hold were charged


@pytest.mark.parametrize("N,T,B,top_n,cutoff_prob", [(3, 17, 10, 40, 1.0), (8, 61, 128, 40, 0.9), (3, 40, 256, 5, 1.0)])
def test_zero_weights_equal_the_entry_without_lm(N, T, B, top_n, cutoff_prob):
    from deepspeech.pytorch_amd import ops
    p, sizes = _inputs(5 + N + T, N, T)
    view, sz = torch.from_numpy(p).to(DEV), torch.from_numpy(sizes)
    ids, gt = _tables("char3", "|")
    m = _lm("char3")
    a = ops.beam_decode(view, sz, 0, B, top_n, cutoff_prob)
    b = ops.beam_decode_clm(view, sz, 0, B, top_n, cutoff_prob, ids, gt, m.order, m.bos, 0.0, 0.0)
    assert a[0] == b[0]
    assert all(torch.equal(x, y) for u, v in zip(a[1], b[1]) for x, y in zip(u, v))
    assert torch.equal(_bits(a[2]), _bits(b[2])) and torch.equal(_bits(b[2]), _bits(b[3]))


def _flip_input():
    """THE HAT, one label per two frames with a blank between, logits +-6, and Q raised 0.4 above H at its frame"""
    labels = _labels()
    frames = []
    for ch in "THE HAT":
        frames += [labels.index(ch), 0]
    z = np.full((len(frames), len(labels)), -6.0)
    z[np.arange(len(frames)), frames] = 6.0
    t = [i for i, c in enumerate(frames) if c == labels.index("H")][1]
    z[t, labels.index("Q")] = 6.4
    return _softmax(z)[None]


def test_character_model_flips_a_planted_misspelling():
    from deepspeech.pytorch_amd.decoder import BeamCTCDecoder
    labels = _labels()
    p = _flip_input()
    T = p.shape[1]
    text = lambda lab: ''.join(labels[c] for c in lab)
    # on the CPU first
    plain = beam_search(p[0], T, 0, 16, 40, 1.0)["beams"]
    assert text(plain[0][0]) == "THE QAT"
    ref = beam_search_clm(p[0], T, 0, 16, 40, 1.0, CharScorer(_lm("char3"), labels, 0, 1.0, 0.0, "|"))["beams"]
    assert text(ref[0][0]) == "THE HAT"
    # then on the device
    probs = torch.from_numpy(p).to(DEV)
    assert BeamCTCDecoder(labels, beam_width=16).decode(probs)[0][0][0] == "THE QAT"
    dec = BeamCTCDecoder(labels, _path("char3"), 1.0, 0.0, beam_width=16, lm_unit="char", space_token="|")
    strings, offsets, scores, acoustic = dec.decode_beams_detailed(probs)
    assert strings[0][0] == "THE HAT" and len(offsets[0][0]) == 7
    assert float(acoustic[0, 0]) > float(plain[0][2])                    # acoustically worse than the misspelling
    auto = BeamCTCDecoder(labels, _path("char3"), 1.0, 0.0, beam_width=16, lm_unit="auto", space_token="|")
    assert auto.lm_unit == "char" and auto.decode(probs)[0][0][0] == "THE HAT"


def test_label_set_without_a_space():
    """the CJK labels hold no space: the constructor takes them in character mode, and the decoder follows the model"""
    from deepspeech.pytorch_amd.decoder import BeamCTCDecoder
    dec = BeamCTCDecoder(CJK_LABELS, _path("cjk3"), 1.0, 0.5, cutoff_top_n=64, beam_width=64, lm_unit="char")
    assert dec.lm_unit == "char" and dec.space_index == len(CJK_LABELS)
    case = GRID[-1]
    p, sizes, refs = _case(*case)
    strings, offsets, scores = dec.decode_beams(torch.from_numpy(p).to(DEV), torch.from_numpy(sizes))
    for n, ref in enumerate(refs):
        assert strings[n][0] == ''.join(CJK_LABELS[c] for c in ref["beams"][0][0]) and len(strings[n][0]) > 5
        assert tuple(offsets[n][0].tolist()) == ref["beams"][0][1]


# ---- streams ----------------------------------------------------------------------------------------------------------------------
class StreamCase:
    """one character-LM configuration on one input: the one-shot oracle per slice, computed once and shared"""

    def __init__(self, p, B, order=3, top_n=40, cutoff_prob=1.0, alpha=1.3, beta=0.7):
        self.p = torch.from_numpy(p).to(DEV)
        self.C, self.B, self.top_n, self.cutoff_prob = p.shape[2], B, top_n, cutoff_prob
        ids, gt = _tables(FILES[order], "|")
        m = _lm(FILES[order])
        self.lm = dict(unit="char", label_ids=ids, ngram_table=gt, order=m.order, bos=m.bos, alpha=alpha, beta=beta)
        self._oracle = {}

    def chunk(self, pos, sizes, nan=True):
        x = torch.full((len(sizes), max(max(sizes), 1), self.C), float("nan") if nan else 0.0, device=DEV)
        for i, (a, s) in enumerate(zip(pos, sizes)):
            x[i, :s] = self.p[i, a:a + s]
        return x

    def oneshot(self, t, start=None):
        from deepspeech.pytorch_amd import ops
        start = tuple(start) if start is not None else (0,) * len(t)
        key = (tuple(t), start)
        if key not in self._oracle:
            L = self.lm
            self._oracle[key] = ops.beam_decode_clm(self.chunk(start, t, nan=False), torch.tensor(list(t), dtype=torch.int32), 0,
                                                    self.B, self.top_n, self.cutoff_prob, L["label_ids"], L["ngram_table"],
                                                    L["order"], L["bos"], L["alpha"], L["beta"])
        return self._oracle[key]


ST_T = 61
ST_TOTALS = (ST_T, 0, ST_T - 11)                       # stream 1 is left at 0 frames


@functools.lru_cache(maxsize=None)
def _stream_case(B):
    p, _ = _inputs(31, 3, ST_T)
    return StreamCase(p, B)


def _feeds(totals, chunks):
    feeds, done, i = [], [0] * len(totals), 0
    while any(d < t for d, t in zip(done, totals)):
        c = chunks[min(i, len(chunks) - 1)]
        s = [min(c, t - d) for d, t in zip(done, totals)]
        feeds.append(tuple(s))
        done = [d + v for d, v in zip(done, s)]
        i += 1
    return feeds


@pytest.mark.parametrize("chunks", [(1,), (7,), (20, 41), (ST_T,)], ids=lambda c: "x".join(str(v) for v in c))
@pytest.mark.parametrize("B", [4, 16, 256])
def test_every_prefix_of_a_stream_equals_the_one_shot_call(B, chunks):
    from deepspeech.pytorch_amd import ops
    case = _stream_case(B)
    h = ops.beam_stream_open(3, ST_T, case.C, 0, B, case.top_n, case.cutoff_prob, DEV, case.lm)
    assert h.flags == 5
    done = [0] * 3
    for s in _feeds(ST_TOTALS, chunks):
        assert ops.beam_stream_feed(h, case.chunk(done, s), torch.tensor(s, dtype=torch.int32)) is None
        done = [d + v for d, v in zip(done, s)]
        _same(ops.beam_stream_result(h, max(done)), case.oneshot(done))
    hdr = ops.beam_stream_header(h)
    assert hdr[:, 0].tolist() == list(ST_TOTALS) and hdr[:, 2].tolist() == [0, 0, 0]


def test_reset_of_one_stream_between_feeds():
    from deepspeech.pytorch_amd import ops
    case = _stream_case(16)
    h = ops.beam_stream_open(3, ST_T, case.C, 0, 16, case.top_n, case.cutoff_prob, DEV, case.lm)
    ops.beam_stream_feed(h, case.chunk([0, 0, 0], (20, 0, 20)), torch.tensor([20, 0, 20], dtype=torch.int32))
    ops.beam_stream_reset(h, [2])
    ops.beam_stream_feed(h, case.chunk([20, 0, 20], (41, 0, 30)), torch.tensor([41, 0, 30], dtype=torch.int32))
    _same(ops.beam_stream_result(h, ST_T), case.oneshot((61, 0, 30), (0, 0, 20)))


# ---- endpointed streams -----------------------------------------------------------------------------------------------------------
EP_SENTENCES = ["THE CAT SAT ON THE MAT ", "IT'S A BIG RED HAT ", "THEY SAT IN THE TENT ", "AT TEN SHE ATE A NUT "]
# four streams of about 70 frames with two planted pauses each (S speech, b silent; endpoint_reference's letters)
EP_SCHEDULES = ("S" * 20 + "bbbb" + "S" * 22 + "bbbbb" + "S" * 19,
                "bb" + "S" * 17 + "bbb" + "S" * 30 + "bbbb" + "S" * 12,
                "S" * 9 + "bbbbbb" + "S" * 25 + "bbb" + "S" * 27,
                "S" * 31 + "bbb" + "S" * 14 + "bbbb" + "S" * 16 + "bb")


class EndpointCase:
    def __init__(self, B):
        import endpoint_reference as R
        from deepspeech.pytorch_amd.decoder import BeamCTCDecoder
        self.labels = _labels()
        path = [[self.labels.index(ch) for ch in s] for s in EP_SENTENCES]
        self.np = R.planted_probs(len(self.labels), 17, schedules=EP_SCHEDULES, path=path)
        self.p = torch.from_numpy(self.np).to(DEV)
        self.totals = [len(s) for s in EP_SCHEDULES]
        self.sil = [R.silent_mask(self.np[n, :self.totals[n], 0], R.THRESHOLD) for n in range(4)]
        self.dec = BeamCTCDecoder(self.labels, _path("char3"), 1.3, 0.7, beam_width=B, lm_unit="char", space_token="|")
        self.B = B
        self._oracle = {}

    def oneshot(self, n, a, b):
        """ops.beam_decode_clm on probs[n, a:b]"""
        from deepspeech.pytorch_amd import ops
        if (n, a, b) not in self._oracle:
            x = torch.zeros((1, max(b - a, 1), self.p.shape[2]), device=DEV)
            x[0, :b - a] = self.p[n, a:b]
            L = self.dec._lm_args(self.p.device)
            self._oracle[(n, a, b)] = ops.beam_decode_clm(x, torch.tensor([b - a], dtype=torch.int32), 0, self.B, 40, 1.0,
                                                          L["label_ids"], L["ngram_table"], L["order"], L["bos"], L["alpha"], L["beta"])
        return self._oracle[(n, a, b)]


@functools.lru_cache(maxsize=None)
def _endpoint_case(B):
    return EndpointCase(B)


@pytest.mark.parametrize("step", [3, 7])
@pytest.mark.parametrize("B", [4, 16])
def test_endpointed_segments_and_partials_equal_the_one_shot_call_on_their_frames(B, step):
    import endpoint_reference as R
    from deepspeech.pytorch_amd.decoder import Endpointer
    case = _endpoint_case(B)
    rule = (R.MIN_TRAILING, R.MAX_LEADING, R.MAX_SEGMENT)
    st = case.dec.stream(4, R.MAX_SEGMENT, DEV, endpoint=Endpointer(R.THRESHOLD, *rule), nbest=4)
    walk = [R.Walker(*rule) for _ in range(4)]
    done, got = [0] * 4, [[] for _ in range(4)]
    for s in _feeds(case.totals, (step,)):
        x = torch.full((4, max(s), case.p.shape[2]), float("nan"), device=DEV)
        for n in range(4):
            x[n, :s[n]] = case.p[n, done[n]:done[n] + s[n]]
            for v in case.sil[n][done[n]:done[n] + s[n]]:
                walk[n].step(bool(v))
        st.feed(x, list(s))
        done = [d + v for d, v in zip(done, s)]
        text, offs = st.best()
        for n in range(4):
            toks, fr, _, _ = case.oneshot(n, walk[n].start, done[n])
            assert text[n] == ''.join(case.labels[c] for c in toks[0][0]), (n, done)
            assert torch.equal(offs[n] - walk[n].start, fr[0][0].to(torch.int)), (n, done)
        for n, segs in enumerate(st.segments()):
            got[n] += segs
    st.end()
    for n, segs in enumerate(st.segments()):
        got[n] += segs
    for n in range(4):
        assert [(g.start, g.end, g.reason) for g in got[n]] == R.segments_walk(case.sil[n], *rule), n
        assert len(got[n]) >= 3
        for seg in got[n]:
            toks, fr, sc, ac = case.oneshot(n, seg.start, seg.end + 1)
            assert seg.labels == toks[0][:4], (n, seg)
            assert all(torch.equal(o - seg.start, f.to(torch.int)) for o, f in zip(seg.offsets, fr[0]))
            assert torch.equal(_bits(seg.scores), _bits(sc[0, :4])) and torch.equal(_bits(seg.acoustic), _bits(ac[0, :4])), (n, seg)
    assert any(seg.strings[0] for segs in got for seg in segs)


# ---- the weight grid --------------------------------------------------------------------------------------------------------------
POINTS = [(0.0, 0.0), (1.0, 0.0), (0.5, 1.5), (2.0, 0.3), (1.3, -0.4), (0.1, 2.5)]


@pytest.mark.parametrize("B", [10, 128])
def test_grid_rank_0_equals_the_single_point_call(B):
    from deepspeech.pytorch_amd import ops
    p, sizes = _inputs(11, 3, 17)
    view, sz = torch.from_numpy(p).to(DEV), torch.from_numpy(sizes)
    ids, gt = _tables("char3", "|")
    m = _lm("char3")
    toks, offs, lens, scores, acoustic = ops.beam_decode_clm_grid(view, sz, 0, B, 40, 1.0, ids, gt, m.order, m.bos,
                                                                  [a for a, _ in POINTS], [b for _, b in POINTS])
    assert toks.shape == (6, 3, 17) and scores.shape == (6, 3)
    lens, toks, offs, scores, acoustic = lens.cpu(), toks.cpu(), offs.cpu(), scores.cpu(), acoustic.cpu()
    for g, (al, be) in enumerate(POINTS):
        one = ops.beam_decode_clm(view, sz, 0, B, 40, 1.0, ids, gt, m.order, m.bos, al, be)
        for n in range(3):
            L = int(lens[g, n])
            assert toks[g, n, :L].tolist() == one[0][n][0] and torch.equal(offs[g, n, :L], one[1][n][0])
        assert torch.equal(_bits(scores[g]), _bits(one[2][:, 0])) and torch.equal(_bits(acoustic[g]), _bits(one[3][:, 0]))
    plain = ops.beam_decode(view, sz, 0, B, 40, 1.0)
    for n in range(3):
        assert toks[0, n, :int(lens[0, n])].tolist() == plain[0][n][0]
    assert torch.equal(_bits(scores[0]), _bits(plain[2][:, 0]))
    # the decoder's form of the same call
    from deepspeech.pytorch_amd.decoder import BeamCTCDecoder
    dec = BeamCTCDecoder(_labels(), _path("char3"), beam_width=B, lm_unit="char", space_token="|")
    strings, _, sc = dec.decode_grid(view, sz, POINTS)
    assert torch.equal(_bits(sc), _bits(scores))
    assert strings[1][0] == ''.join(_labels()[c] for c in toks[1, 0, :int(lens[1, 0])].tolist())


# ---- words and confidence ---------------------------------------------------------------------------------------------------------
def test_decode_words_in_character_mode():
    from deepspeech.pytorch_amd import ops
    from deepspeech.pytorch_amd.confidence import Confidence
    from deepspeech.pytorch_amd.decoder import BeamCTCDecoder
    labels = _labels()
    p, sizes = _inputs(77, 3, 40)
    pd, sz = torch.from_numpy(p).to(DEV), torch.from_numpy(sizes)
    dec = BeamCTCDecoder(labels, _path("char3"), 1.2, 0.8, beam_width=8, lm_unit="char", space_token="|")
    strings, offsets, scores, acoustic = dec.decode_beams_detailed(pd, sz)
    for conf in (Confidence(), Confidence("max_prob", aggregate="prod", word_aggregate="mean"),
                 Confidence("entropy", aggregate="min", word_aggregate="mean")):
        out = dec.decode_words(pd, sz, confidence=conf, nbest=2)
        assert len(out) == 3 and all(len(o) == 2 for o in out)
        # ops.confidence on the tokens of decode_beams_detailed
        width = max(max(len(strings[n][r]) for n in range(3) for r in range(2)), 1)
        tk = torch.zeros((3, 2, width), dtype=torch.int32)
        of = torch.zeros((3, 2, width), dtype=torch.int32)
        ln = torch.zeros((3, 2), dtype=torch.int32)
        for n in range(3):
            for r in range(2):
                L = len(strings[n][r])
                tk[n, r, :L] = torch.tensor([labels.index(c) for c in strings[n][r]], dtype=torch.int32)
                of[n, r, :L] = offsets[n][r]
                ln[n, r] = L
        want = [t.cpu() for t in ops.confidence(pd, sz, tk.to(DEV), of.to(DEV), ln.to(DEV), 0, dec.space_index, conf.measure,
                                                conf.alpha, conf.aggregate, conf.word_aggregate)]
        f32 = lambda v: np.float32(v).tobytes()
        for n in range(3):
            for r, h in enumerate(out[n]):
                assert h.text == strings[n][r]
                assert f32(h.score) == scores[n, r].numpy().tobytes() and f32(h.acoustic) == acoustic[n, r].numpy().tobytes()
                L, W = len(h.text), int(want[8][n, r])
                assert [c.start_frame for c in h.chars] == want[0][n, r, :L].tolist()
                assert [c.end_frame for c in h.chars] == want[1][n, r, :L].tolist()
                assert [f32(c.confidence) for c in h.chars] == [f32(v) for v in want[2][n, r, :L].tolist()]
                assert len(h.words) == W
                assert [w.start_frame for w in h.words] == want[5][n, r, :W].tolist()
                assert [w.end_frame for w in h.words] == want[6][n, r, :W].tolist()
                assert [f32(w.confidence) for w in h.words] == [f32(v) for v in want[7][n, r, :W].tolist()]
                if W:
                    assert f32(h.confidence) == f32(float(want[9][n, r]))
    assert any(len(h.words) > 1 for o in out for h in o)


def test_stream_words_and_sessions_take_the_character_decoder():
    """BeamStream with confidence= and nbest through decoder.stream: words() equals decode_words on the frames so far"""
    from deepspeech.pytorch_amd.confidence import Confidence
    from deepspeech.pytorch_amd.decoder import BeamCTCDecoder
    labels = _labels()
    p, _ = _inputs(78, 2, 30)
    pd = torch.from_numpy(p).to(DEV)
    dec = BeamCTCDecoder(labels, _path("char3"), 1.2, 0.8, beam_width=8, lm_unit="char", space_token="|")
    st = dec.stream(2, 30, DEV, confidence=Confidence())
    for a, b in ((0, 11), (11, 30)):
        st.feed(pd[:, a:b])
        got = st.words(nbest=2)
        want = dec.decode_words(pd[:, :b], None, Confidence(), nbest=2)
        for n in range(2):
            for g, w in zip(got[n], want[n]):
                assert g.text == w.text and g.score == w.score and g.acoustic == w.acoustic
                assert [(c.start_frame, c.end_frame, c.confidence) for c in g.chars] == \
                    [(c.start_frame, c.end_frame, c.confidence) for c in w.chars]
                assert [(x.text, x.confidence) for x in g.words] == [(x.text, x.confidence) for x in w.words]
        strings, _, scores = st.result()
        one = dec.decode_beams(pd[:, :b])
        assert strings == one[0] and torch.equal(_bits(scores), _bits(one[2]))


def test_streaming_transcriber_and_stream_pool_take_the_character_decoder():
    """the sessions only call decoder.stream: their words equal decode_words of the character decoder on their own probabilities"""
    from test_gpu_confidence import _hyp_key, _session_case
    from deepspeech.pytorch_amd.confidence import Confidence
    from deepspeech.pytorch_amd.decoder import BeamCTCDecoder
    from deepspeech.pytorch_amd.streaming import StreamingTranscriber, StreamPool
    fx, m, x, lengths, chunks = _session_case()
    dec = BeamCTCDecoder(fx.labels, _path("char3"), 0.6, 0.4, beam_width=8, lm_unit="char", space_token="|")
    conf = Confidence()
    st = StreamingTranscriber(m, dec, carry_context=True, max_frames=80, confidence=conf)
    pos, outs = 0, [[] for _ in lengths]
    for i, c in enumerate(chunks):
        last = i == len(chunks) - 1
        st.feed(x[:, :, :, pos:pos + c].contiguous(), [g - pos for g in lengths] if last else [c] * len(lengths), final=last)
        if st.last_output is not None:
            probs, sizes = st.last_output
            for n in range(len(lengths)):
                outs[n].append(probs[n, :int(sizes[n])])
        pos += c
    got = st.words()
    for n in range(len(lengths)):
        pn = torch.cat(outs[n])[None]
        assert pn.shape[1] == st.frames[n] > 0
        assert [_hyp_key(h) for h in got[n]] == [_hyp_key(h) for h in dec.decode_words(pn, None, conf)[0]]
    pool = StreamPool(m, dec, 2, max_frames=80, confidence=conf)
    slot = pool.open()
    fed, outs = 0, []
    for c in chunks:
        c = min(c, lengths[0] - fed)
        pool.feed([slot], x[:1, :, :, fed:fed + c].contiguous(), [c], final=[slot] if fed + c == lengths[0] else [])
        if pool.last_output.get(slot) is not None:
            outs.append(pool.last_output[slot])
        fed += c
    pk = torch.cat(outs)[None]
    assert pk.shape[1] == pool.frames(slot) > 0
    assert [_hyp_key(h) for h in pool.words(slot, nbest=2)] == [_hyp_key(h) for h in dec.decode_words(pk, None, conf, nbest=2)[0]]


# ---- argument errors --------------------------------------------------------------------------------------------------------------
def test_argument_errors():
    from deepspeech.pytorch_amd import _lib, ops
    labels = _labels()
    ids, gt = _tables("char3", "|")
    m = _lm("char3")
    p = torch.from_numpy(_inputs(1, 2, 10)[0]).to(DEV)
    good = dict(probs=p, sizes=None, blank=0, beam_width=4, cutoff_top_n=40, cutoff_prob=1.0, label_ids=ids, ngram_table=gt,
                order=m.order, bos=m.bos, alpha=1.0, beta=1.0)
    ops.beam_decode_clm(**good)
    bads = (dict(order=6), dict(order=0), dict(beam_width=257), dict(label_ids=ids[:5]), dict(label_ids=ids.cpu()),
            dict(label_ids=ids.to(torch.int64)), dict(label_ids=None), dict(ngram_table=gt.cpu()), dict(ngram_table=gt[:3]),
            dict(bos=-1))
    for bad in bads:
        with pytest.raises(ValueError):
            ops.beam_decode_clm(**dict(good, **bad))
    grid = {k: v for k, v in good.items() if k not in ("alpha", "beta")}
    ops.beam_decode_clm_grid(alphas=[1.0, 0.5], betas=[0.0, 1.0], **grid)
    for bad in bads + (dict(alphas=[1.0]), dict(alphas=[], betas=[])):
        with pytest.raises(ValueError):
            ops.beam_decode_clm_grid(**dict(dict(grid, alphas=[1.0, 0.5], betas=[0.0, 1.0]), **bad))
    lm = dict(unit="char", label_ids=ids, ngram_table=gt, order=m.order, bos=m.bos, alpha=1.0, beta=1.0)
    ops.beam_stream_open(2, 10, len(labels), 0, 4, 40, 1.0, DEV, lm)
    for bad in (dict(order=6), dict(label_ids=ids[:5]), dict(ngram_table=gt.cpu()), dict(unit="syllable")):
        with pytest.raises(ValueError):
            ops.beam_stream_open(2, 10, len(labels), 0, 4, 40, 1.0, DEV, dict(lm, **bad))
    with pytest.raises(ValueError, match="hot words"):
        ops.beam_stream_open(2, 10, len(labels), 0, 4, 40, 1.0, DEV, lm, dict(space=len(labels) - 1, table=gt))
    # the raw ABI
    lib = _lib.load()
    N, T, C, B = 2, 10, len(labels), 4
    buf = torch.empty((2, N, B, T), dtype=torch.int32, device=DEV)
    lens = torch.empty((N, B), dtype=torch.int32, device=DEV)
    scores = torch.empty((N, B), dtype=torch.float32, device=DEV)
    ws = torch.empty(lib.ds2_beam_ws_bytes(N, T, B), dtype=torch.uint8, device=DEV)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def raw(cid=ids.data_ptr(), gtab=gt.data_ptr(), gslots=gt.shape[0], order=m.order):
        return lib.ds2_beam_decode_clm(p.data_ptr(), p.stride(0), p.stride(1), N, T, C, None, 0, B, 40, 1.0, cid, gtab, gslots, order,
                                       m.bos, 1.0, 1.0, buf[0].data_ptr(), buf[1].data_ptr(), lens.data_ptr(), scores.data_ptr(), None,
                                       ws.data_ptr(), stream)

    assert raw() == 0
    torch.cuda.synchronize()
    for kw in (dict(cid=None), dict(order=6), dict(order=0), dict(gtab=None), dict(gslots=gt.shape[0] - 1), dict(gslots=0)):
        assert raw(**kw) == 1002, kw                                          # DS2_ERR_ARG
    al = torch.tensor([1.0, 0.5], device=DEV)
    gws = torch.empty(lib.ds2_beam_grid_ws_bytes(2, N, T, B), dtype=torch.uint8, device=DEV)

    def raw_grid(cid=ids.data_ptr(), order=m.order, G=2):
        return lib.ds2_beam_decode_clm_grid(p.data_ptr(), p.stride(0), p.stride(1), N, T, C, None, 0, B, 40, 1.0, cid, gt.data_ptr(),
                                            gt.shape[0], order, m.bos, G, al.data_ptr(), al.data_ptr(), buf[0].data_ptr(),
                                            buf[1].data_ptr(), lens.data_ptr(), scores.data_ptr(), None, gws.data_ptr(), stream)

    assert raw_grid() == 0
    torch.cuda.synchronize()
    assert raw_grid(cid=None) == 1002 and raw_grid(order=6) == 1002 and raw_grid(G=0) == 1002
    state = torch.empty(lib.ds2_beam_stream_bytes(N, B, T, 5), dtype=torch.uint8, device=DEV)
    assert lib.ds2_beam_stream_reset(state.data_ptr(), N, B, T, 5, None, stream) == 0
    assert lib.ds2_beam_stream_reset(state.data_ptr(), N, B, T, 4, None, stream) == 1002
    assert lib.ds2_beam_stream_reset(state.data_ptr(), N, B, T, 7, None, stream) == 1002
    sws = torch.empty(lib.ds2_beam_stream_ws_bytes(N, T), dtype=torch.uint8, device=DEV)

    def raw_feed(cid=ids.data_ptr(), order=m.order):
        return lib.ds2_beam_stream_feed_clm(p.data_ptr(), p.stride(0), p.stride(1), N, T, C, None, 0, B, 40, 1.0, cid, gt.data_ptr(),
                                            gt.shape[0], order, m.bos, 1.0, 1.0, state.data_ptr(), T, None, None, 0, 0, None, None,
                                            None, sws.data_ptr(), stream)

    assert raw_feed(cid=None) == 1002 and raw_feed(order=6) == 1002
    assert raw_feed() == 0
    torch.cuda.synchronize()
