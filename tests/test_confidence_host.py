"""Host checks of the word-timing / confidence rules (include/ds2hip.h "confidence") on their numpy
restatement tests/confidence_reference.py, and of the host bookkeeping of deepspeech/pytorch_amd/confidence.py: the stated
consequences of the span rule, word grouping against str.split, and the argument errors.  No GPU."""
import os
import re

import numpy as np
import pytest
import torch

import confidence_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LABELS = "_ABC "            # blank, three letters, the space
SPACE = 4


@pytest.mark.parametrize("measure", ["entropy", "tsallis", "renyi"])
@pytest.mark.parametrize("C", [2, 4, 29, 65, 130])
def test_uniform_frame_is_0_and_one_hot_frame_is_1(measure, C):
    uniform = np.full(C, 1.0 / C, np.float32)
    # 1/C is rounded to fp32 before the fp64 sums: the value is 0 up to that rounding (2^-24 relative, times ln C / ln C)
    assert abs(float(R.frame_value(uniform, 0, measure, 1 / 3))) <= 1e-6
    if C in (2, 4):
        assert R.frame_value(uniform, 0, "entropy", 1 / 3) == 0.0        # 1/C and its log are exact there
    hot = np.zeros(C, np.float32)
    hot[C // 2] = 1.0
    assert R.frame_value(hot, C // 2, measure, 1 / 3) == 1.0
    assert R.frame_value(hot, C // 2, measure, 2.0) == 1.0


def test_wave_sum_is_the_documented_order():
    v = np.random.default_rng(0).standard_normal(130)
    part = np.zeros(64)
    for j in range(64):
        acc = 0.0
        for c in range(j, len(v), 64):
            acc = acc + v[c]
        part[j] = acc
    for o in (32, 16, 8, 4, 2, 1):
        part = np.array([part[j] + part[j ^ o] for j in range(64)])
    assert R.wave_sum(v) == part[0]
    assert R.wave_sum(np.zeros(0)) == 0.0


def test_first_maximum_and_nan_follow_the_greedy_scan():
    nan = np.float32("nan")
    assert R.argmax_first(np.array([1, 3, 3, 2], np.float32)) == 1
    assert R.argmax_first(np.array([nan, 5, 1], np.float32)) == 0          # the scan starts at class 0 and nothing beats a NaN
    assert R.argmax_first(np.array([1, nan, 5, 5], np.float32)) == 2       # a NaN elsewhere never wins
    assert R.argmax_first(np.array([-np.inf, nan], np.float32)) == 0


def _greedy(a, blank):
    tok, off = [], []
    for t, l in enumerate(a):
        if l != blank and (t == 0 or l != a[t - 1]):
            tok.append(int(l))
            off.append(t)
    return tok, off


def test_greedy_span_is_the_argmax_run():
    rng = np.random.default_rng(1)
    for _ in range(50):
        T = int(rng.integers(1, 40))
        a = rng.integers(0, 4, T)
        a = np.repeat(a, rng.integers(1, 4, T))[:T]
        tok, off = _greedy(a, 0)
        sp = R.spans(a, T, tok, off)
        runs = []
        for t in range(T):
            if a[t] != 0 and (t == 0 or a[t] != a[t - 1]):
                e = t
                while e + 1 < T and a[e + 1] == a[t]:
                    e += 1
                runs.append((t, e))
        assert sp == runs


def test_spans_are_disjoint_and_increasing_for_increasing_offsets():
    rng = np.random.default_rng(2)
    for _ in range(200):
        T = int(rng.integers(1, 50))
        a = rng.integers(0, 3, T)                    # few classes: long runs, many labels that are not the arg-max
        L = int(rng.integers(0, T + 1))
        off = sorted(rng.choice(T, L, replace=False).tolist())
        tok = rng.integers(0, 3, L).tolist()
        sp = R.spans(a, T, tok, off)
        for i, (s, e) in enumerate(sp):
            assert 0 <= s <= off[i] <= e < T
            if i:
                assert s > sp[i - 1][1]


def test_hand_made_non_monotone_offsets_follow_the_rule():
    a = np.array([1, 1, 1, 2, 2, 2, 1, 1])
    # token 1 lies BEFORE token 0: token 0's forward walk is empty (off[1] <= off[0]); token 1 walks forward to its run's end and
    # back only to above token 0's forward end ... which is frame 4, above its own frame: it stays at its frame
    assert R.spans(a, 8, [2, 1], [4, 1]) == [(3, 4), (1, 2)]
    # equal offsets: both tokens sit on frame 3
    assert R.spans(a, 8, [2, 2], [3, 3]) == [(3, 3), (3, 5)]
    # a label that is not the arg-max keeps its own frame only
    assert R.spans(a, 8, [2], [0]) == [(0, 0)]
    # the span ends at sizes - 1
    assert R.spans(a, 7, [1], [6]) == [(6, 6)] and R.spans(a, 8, [1], [6]) == [(6, 7)]


@pytest.mark.parametrize("text", ["AB C", " AB", "AB ", "A  B", "  ", " ", "", "ABC", " A B  CA "])
def test_word_grouping_equals_str_split(text):
    tok = [LABELS.index(ch) for ch in text]
    runs = R.word_runs(tok, SPACE)
    assert [text[f:l + 1] for f, l in runs] == text.split()
    # without a space label the whole hypothesis is one word
    assert R.word_runs(tok, len(LABELS)) == ([(0, len(tok) - 1)] if tok else [])


def test_make_hypothesis_builds_words_chars_and_seconds():
    from deepspeech.pytorch_amd import confidence as Cf
    i2c = dict(enumerate(LABELS))
    labels = [LABELS.index(ch) for ch in "AB C"]
    res = ([0, 2, 5, 6], [1, 4, 5, 8], [0.5, 0.25, 1.0, 0.75], [0, 3], [1, 3], [0, 6], [4, 8], [0.25, 0.75], 2, 0.25)
    h = Cf.make_hypothesis(labels, i2c, SPACE, res, 1.5, 1.25, frame_seconds=0.02, shift=100)
    assert h.text == "AB C" and h.score == 1.5 and h.acoustic == 1.25 and h.confidence == 0.25 and h.labels == labels
    assert [w.text for w in h.words] == h.text.split()
    assert h.words[0] == Cf.Word("AB", 100, 104, 0.25, 100 * 0.02, 105 * 0.02)
    assert h.chars[3] == Cf.Char("C", 106, 108, 0.75, 106 * 0.02, 109 * 0.02)
    e = Cf.make_hypothesis([], i2c, SPACE, ([], [], [], [], [], [], [], [], 0, float("nan")))
    assert e.text == "" and e.confidence is None and e.words == [] and e.chars == []
    assert Cf.make_hypothesis(labels, i2c, SPACE, res).words[0].start_s is None


def test_confidence_argument_errors():
    from deepspeech.pytorch_amd.confidence import Confidence
    c = Confidence()
    assert (c.measure, c.alpha, c.aggregate, c.word_aggregate) == ("label_prob", 1 / 3, "mean", "min")
    assert repr(c) == "Confidence(measure='label_prob', alpha=%r, aggregate='mean', word_aggregate='min')" % (1 / 3)
    for kw in (dict(measure="margin"), dict(aggregate="max"), dict(word_aggregate="sum"), dict(alpha=0), dict(alpha=-1.0),
               dict(alpha=float("nan")), dict(measure="tsallis", alpha=1), dict(measure="renyi", alpha=1.0)):
        with pytest.raises(ValueError):
            Confidence(**kw)
    Confidence(measure="entropy", alpha=1)           # alpha plays no part there
    with pytest.raises(ValueError):
        Confidence(measure="entropy").check_classes(1)
    Confidence(measure="max_prob").check_classes(1)


def test_decode_words_argument_errors():
    from deepspeech.pytorch_amd.confidence import Confidence
    from deepspeech.pytorch_amd.decoder import BeamCTCDecoder, GreedyDecoder
    p = torch.full((1, 3, 5), 0.2)
    g, b = GreedyDecoder(LABELS), BeamCTCDecoder(LABELS, beam_width=4)
    with pytest.raises(ValueError):
        g.decode_words(p, confidence="entropy")
    with pytest.raises(ValueError):
        g.decode_words(p, kind="scores")
    with pytest.raises(ValueError):
        g.decode_words(p[:, :, :1], confidence=Confidence(measure="entropy"))
    with pytest.raises(ValueError):
        b.decode_words(p, confidence=3)
    for nbest in (0, 5):
        with pytest.raises(ValueError):
            b.decode_words(p, nbest=nbest)


def test_ring_capacity_bound_holds_under_simulated_feed_and_fetch_schedules():
    """decoder.ring_capacity against the stream's own pieces: split_feed cuts a feed into device feeds of at most
    Endpointer.sub_feed frames, a fetch happens once RING_SLOTS device feeds have passed since the last one (EndpointedBeamStream.
    _fed_once) or whenever the caller asks.  The endpointing rule (Endpointer's docstring) is walked frame by frame on random
    silence patterns; after every device feed the frames from the start of the oldest segment not yet fetched, or of the open
    one, to the newest frame must fit the ring, the device's ring of finished segments must not overflow, and no device feed may
    hold two endpoints.  A segment that is not yet fetched has its LAST frame inside the window since the last fetch, so the frames needed
    are at most capacity - 1; some schedule must reach exactly that, which shows the capacity is not slack by more than a frame."""
    from deepspeech.pytorch_amd import decoder as D
    assert D.EndpointedBeamStream.RING_SLOTS == D.RING_SLOTS
    rng = np.random.default_rng(3)
    tight = 0
    for trial in range(300):
        ep = D.Endpointer(0.8, int(rng.integers(1, 7)), int(rng.integers(1, 9)), int(rng.integers(1, 13)))
        cap = D.ring_capacity(ep)
        assert cap == ep.max_segment + D.RING_SLOTS * ep.sub_feed
        p_silent = float(rng.random())
        start = frames = n = trailing = since = 0
        spoken, unfetched, worst = False, [], 0
        for _ in range(30):
            chunk = int(rng.integers(0, 3 * cap))
            silent = rng.random(chunk) < p_silent
            for t0, t1, sub in D.split_feed([chunk], ep.sub_feed):
                assert sub[0] == t1 - t0 <= ep.sub_feed
                ends = 0
                for t in range(t0, t1):
                    frames, n = frames + 1, n + 1
                    spoken, trailing = (spoken, trailing + 1) if silent[t] else (True, 0)
                    if (spoken and trailing >= ep.min_trailing) or (not spoken and n >= ep.max_leading) or n >= ep.max_segment:
                        unfetched.append(start)
                        start, n, trailing, spoken, ends = frames, 0, 0, False, ends + 1
                assert ends <= 1 and len(unfetched) <= D.RING_SLOTS
                need = frames - min(unfetched + [start])
                worst = max(worst, need)
                assert need <= cap, (ep, need, cap)
                since += 1
                if since >= D.RING_SLOTS:
                    unfetched, since = [], 0
            if rng.random() < 0.2:                           # the caller drains the segments or asks for the partial
                unfetched, since = [], 0
        tight += worst == cap - 1
    assert tight > 0


def test_word_segment_equals_the_plain_tuple():
    from deepspeech.pytorch_amd.confidence import Hypothesis
    from deepspeech.pytorch_amd.decoder import Segment, WordSegment
    s = Segment(2, 10, 17, "silence", ["AB"], [None], None, None, [[1, 2]])
    h = Hypothesis("AB", 1.0, 1.0, 0.5, [], [], [1, 2])
    w = WordSegment(s, [h])
    assert w == s and tuple(w) == tuple(s) and w._fields == Segment._fields and w.reason == "silence"
    assert w.hypotheses == [h] and w.confidence == 0.5 and WordSegment(s, []).confidence is None


def test_header_declares_the_new_entry_points():
    from deepspeech.pytorch_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "ds2hip.h")).read()
    for name in ("ds2_confidence", "ds2_confidence_ws_bytes", "ds2_frame_store_append"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.SIGNATURES
