"""GPU checks of word timings and confidence (csrc/ds2_confidence.hip, ops.confidence, the decoders' decode_words and the
streams' words) against the numpy restatement of the rules, tests/confidence_reference.py.

Rule of comparison.  Spans, word tables and counts: exact.  label_prob and max_prob on probabilities contain no transcendental:
every confidence is bit-equal.  The entropy measures and kind = logits / log_probs evaluate fp64 expressions on both sides (at
most a few C * 2^-53 of absolute error each, below 1e-13 at these C) and round once, so a FRAME value differs by at most one fp32
ulp, or 1e-12 near 0; the aggregates of such values (all in [0, 1]) are held to 2 * 2^-23 for mean and min and to n * 2^-23 for a
product of n frame values.  Frame values are read through a probe hypothesis with one token on every frame: its spans are single
frames by the span rule, so its token confidences ARE the frame values.  The worst differences seen are printed."""
import functools
import os

import numpy as np
import pytest
import torch

import beam_hot_cases as HC
import confidence_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -23
EXACT = [("label_prob", "mean", "min"), ("label_prob", "prod", "mean"), ("label_prob", "min", "prod"),
         ("max_prob", "mean", "mean"), ("max_prob", "min", "min"), ("max_prob", "prod", "prod")]
# (kind, measure, alpha, aggregate, word_aggregate): the combinations whose aggregates the bounds above are worked out for
CLOSE = [("probs", "entropy", 1 / 3, "mean", "min"), ("probs", "tsallis", 1 / 3, "min", "mean"), ("probs", "renyi", 2.0, "prod", "prod"),
         ("probs", "tsallis", 2.0, "mean", "min"), ("probs", "renyi", 1 / 3, "mean", "min"),
         ("logits", "label_prob", 1 / 3, "mean", "min"), ("logits", "max_prob", 1 / 3, "prod", "prod"),
         ("logits", "entropy", 1 / 3, "min", "mean"), ("log_probs", "label_prob", 1 / 3, "prod", "prod"),
         ("log_probs", "max_prob", 1 / 3, "mean", "min"), ("log_probs", "renyi", 1 / 3, "min", "mean")]
WORST = {"frame_ulp": 0.0, "agg": 0.0}


def _gen_hyp(rng, size, C, space, L, monotone):
    if monotone:
        off = sorted(rng.choice(size, L, replace=False).tolist())
    else:
        off = rng.integers(0, size, L).tolist()
    tok = rng.integers(1, C, L)
    if space < C:
        tok[rng.random(L) < 0.2] = space
        if L >= 67:
            tok[62:67] = 1                       # a word across the 64-token chunk seam
    return tok.tolist(), off


def _greedy(a):
    tok, off = [], []
    for t, l in enumerate(a):
        if l != 0 and (t == 0 or l != a[t - 1]):
            tok.append(int(l))
            off.append(t)
    return tok, off


@functools.lru_cache(maxsize=None)
def _case(Tp, C, lens2=None, B=3):
    """logits z [3][Tp][C] with planted runs, sizes (Tp, below Tp, 0), and B hypotheses per clip: the per-frame probe, the greedy
    hypothesis, and one made by hand (clip 0: non-monotone offsets, clip 1: an invalid one, clip 2 has no frames: any token is
    invalid).  lens2: lengths of the hand-made hypotheses of clips 0 and 1 in place of the default."""
    rng = np.random.default_rng(1000 * Tp + C)
    sizes = [Tp, max(1, Tp - 3), 0]
    space = C - 1 if C >= 4 else C
    z = (rng.standard_normal((3, Tp, C)) * 1.5).astype(np.float32)
    for n in range(3):
        t = 0
        while t < Tp:
            run, l = int(rng.integers(1, 5)), int(rng.integers(0, C))
            z[n, t:t + run, l] += 5.0
            t += run
        if sizes[n]:
            z[n, sizes[n] - 1, 1] += 20.0          # the last valid frame is a label: a span ends at sizes[n] - 1
    hyps = []
    for n in range(3):
        a = z[n, :sizes[n]].argmax(-1)
        probe = (a.tolist(), list(range(sizes[n])))
        hand = ([1], [0])
        if n == 0:
            hand = _gen_hyp(rng, sizes[0], C, space, int(rng.integers(2, sizes[0] + 2)) if Tp > 1 else 1, False)
        elif n == 1:
            tok, off = _gen_hyp(rng, sizes[1], C, space, min(3, sizes[1]), True)
            bad = int(rng.integers(0, 4))
            if bad == 0:
                tok[-1] = C
            elif bad == 1:
                off[-1] = sizes[1]
            elif bad == 2:
                tok[0] = -1
            else:
                off[0] = -1
            hand = (tok, off)
        hyps.append([probe, _greedy(a), hand][:B] if B > 1 else [_greedy(a)])
    if lens2 is not None:
        for n in range(2):
            hyps[n] = [_gen_hyp(rng, sizes[n], C, space, L, L <= sizes[n] and L % 2 == 1) for L in lens2[n]]
    return z, sizes, space, hyps


def _x_of(z, kind):
    if kind == "logits":
        return z
    zz = z.astype(np.float64)
    lp = zz - np.log(np.exp(zz - zz.max(-1, keepdims=True)).sum(-1, keepdims=True)) - zz.max(-1, keepdims=True)
    return lp.astype(np.float32) if kind == "log_probs" else np.exp(lp).astype(np.float32)


def _run(x, sizes, space, hyps, kind, measure, alpha, agg, wagg, lens_override=None):
    from deepspeech.pytorch_amd import ops
    N, B = len(hyps), len(hyps[0])
    ld = max(1, max(len(h[0]) for hs in hyps for h in hs))
    tok = np.full((N, B, ld), -7, np.int32)
    off = np.full((N, B, ld), -7, np.int32)
    lens = np.zeros((N, B), np.int32)
    for n in range(N):
        for b in range(B):
            t, o = hyps[n][b]
            tok[n, b, :len(t)], off[n, b, :len(o)], lens[n, b] = t, o, len(t)
    if lens_override:
        for (n, b), v in lens_override.items():
            lens[n, b] = v
    out = ops.confidence(torch.from_numpy(x).to(DEV), torch.tensor(sizes, dtype=torch.int32), torch.from_numpy(tok).to(DEV),
                         torch.from_numpy(off).to(DEV), torch.from_numpy(lens).to(DEV), 0, space, measure, alpha, agg, wagg, kind)
    return [o.cpu().numpy() for o in out]


def _same_bits(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return bool(np.all((a.view(np.int32) == b.view(np.int32)) | (np.isnan(a) & np.isnan(b))))


def _ulps(a, b):
    """|a - b| in units of the larger one's fp32 ulp"""
    return abs(float(a) - float(b)) / float(np.spacing(np.float32(max(abs(float(a)), abs(float(b)), 1e-38))))


def _check_hyp(out, n, b, ref, exact, agg, wagg, probe):
    ts, te, tc, wf, wl, ws, we, wc, cnt, utt = [o[n, b] for o in out]
    L = len(ref["tok_start"])
    ld, lw = ts.shape[0], wf.shape[0]
    # every element is written: the tails say "nothing here"
    assert (ts[L:] == -1).all() and (te[L:] == -1).all() and np.isnan(tc[L:]).all()
    W = len(ref["words"])
    assert cnt == W
    assert (wf[W:] == -1).all() and (wl[W:] == -1).all() and (ws[W:] == -1).all() and (we[W:] == -1).all() and np.isnan(wc[W:]).all()
    assert ts[:L].tolist() == ref["tok_start"] and te[:L].tolist() == ref["tok_end"]
    assert [(int(wf[w]), int(wl[w]), int(ws[w]), int(we[w])) for w in range(W)] == [tuple(w[:4]) for w in ref["words"]]
    rtc, rwc = np.array(ref["tok_conf"], np.float32), np.array([w[4] for w in ref["words"]], np.float32)
    if exact:
        assert _same_bits(tc[:L], rtc) and _same_bits(wc[:W], rwc) and _same_bits(utt, ref["utt_conf"])
        return
    span = [e - s + 1 for s, e in zip(ref["tok_start"], ref["tok_end"])]
    for i in range(L):
        d = abs(float(tc[i]) - float(rtc[i]))
        if probe or span[i] == 1:                      # a frame value as it is
            WORST["frame_ulp"] = max(WORST["frame_ulp"], _ulps(tc[i], rtc[i]) if d > 1e-12 else 0.0)
            assert d <= 1e-12 or _ulps(tc[i], rtc[i]) <= 1.0, (n, b, i, tc[i], rtc[i])
        else:
            WORST["agg"] = max(WORST["agg"], d / U)
            assert d <= (span[i] * U if agg == "prod" else 2 * U), (n, b, i, tc[i], rtc[i])
    frames = 0
    for w, (f, l, _, _, _) in enumerate(ref["words"]):
        nf = sum(span[f:l + 1])
        frames += nf
        d = abs(float(wc[w]) - float(rwc[w]))
        WORST["agg"] = max(WORST["agg"], d / U)
        assert d <= (nf * U if wagg == "prod" else 2 * U), (n, b, w, wc[w], rwc[w])
    if W:
        d = abs(float(utt) - float(ref["utt_conf"]))
        assert d <= (frames * U if wagg == "prod" else 2 * U), (n, b, utt, ref["utt_conf"])
    else:
        assert np.isnan(utt)


def _check_invalid(out, n, b):
    ts, te, tc, wf, wl, ws, we, wc, cnt, utt = [o[n, b] for o in out]
    assert (ts == -1).all() and (te == -1).all() and np.isnan(tc).all() and cnt == 0 and np.isnan(utt)
    assert (wf == -1).all() and (wl == -1).all() and (ws == -1).all() and (we == -1).all() and np.isnan(wc).all()


@functools.lru_cache(maxsize=None)
def _frames(key, kind, measure, alpha):
    z, sizes, _, _ = _case(*key)
    x = _x_of(z, kind)
    return [R.frame_pass(x[n], sizes[n], kind, measure, alpha) for n in range(len(sizes))]


def _compare(key, kind, measure, alpha, agg, wagg, exact, probe_b=0):
    z, sizes, space, hyps = _case(*key)
    x = _x_of(z, kind)
    out = _run(x, sizes, space, hyps, kind, measure, alpha, agg, wagg)
    fr = _frames(key, kind, "max_prob" if measure == "label_prob" else measure, alpha)
    for n in range(len(hyps)):
        for b, (tok, off) in enumerate(hyps[n]):
            ref = R.hypothesis(x[n], sizes[n], kind, tok, off, space, measure, alpha, agg, wagg, frames=fr[n])
            if ref["valid"]:
                _check_hyp(out, n, b, ref, exact, agg, wagg, probe=(b == probe_b and len(hyps[n]) == 3 and key[2:] == ()))
            else:
                _check_invalid(out, n, b)
    return out


# T' on both sides of the 64-frame and 64-token seams; C = 2, 29 and both sides of the frame kernel's lane seams (64, 128)
SHAPES = [(1, 29), (63, 2), (64, 29), (65, 63), (65, 64), (130, 65), (33, 127), (63, 128), (64, 129)]
SEAM = (130, 5, ((130, 64, 1), (65, 63, 0)))


@pytest.mark.parametrize("Tp,C", SHAPES)
def test_kernel_is_bit_equal_on_probabilities(Tp, C):
    for measure, agg, wagg in EXACT:
        _compare((Tp, C), "probs", measure, 1 / 3, agg, wagg, exact=True)


@pytest.mark.parametrize("measure,agg,wagg", EXACT)
def test_words_and_spans_across_the_token_chunk_seam(measure, agg, wagg):
    z, sizes, space, hyps = _case(*SEAM)
    assert sorted(len(h[0]) for hs in hyps[:2] for h in hs) == [0, 1, 63, 64, 65, 130]
    tok = hyps[0][0][0]
    assert all(t != space for t in tok[62:67])               # the word that spans the seam
    _compare(SEAM, "probs", measure, 1 / 3, agg, wagg, exact=True)


@pytest.mark.parametrize("kind,measure,alpha,agg,wagg", CLOSE)
def test_kernel_is_within_an_ulp_per_frame_elsewhere(kind, measure, alpha, agg, wagg):
    for Tp, C in [(65, 2), (64, 29), (20, 63), (33, 64), (20, 65), (20, 127), (20, 128), (20, 129)]:
        _compare((Tp, C), kind, measure, alpha, agg, wagg, exact=False)
    _compare(SEAM, kind, measure, alpha, agg, wagg, exact=False, probe_b=-1)
    print("worst frame difference %.2f ulp, worst aggregate difference %.2f * 2^-23" % (WORST["frame_ulp"], WORST["agg"]))


def test_one_hypothesis_per_clip_and_lengths_that_cannot_be_trusted():
    _compare((65, 29, None, 1), "probs", "label_prob", 1 / 3, "mean", "min", exact=True)
    z, sizes, space, hyps = _case(64, 29)
    x = _x_of(z, "probs")
    out = _run(x, sizes, space, hyps, "probs", "label_prob", 1 / 3, "mean", "min", lens_override={(0, 1): -1, (1, 0): 65})
    _check_invalid(out, 0, 1)                                # a negative length
    _check_invalid(out, 1, 0)                                # a length beyond the row
    fr = _frames((64, 29), "probs", "max_prob", 1 / 3)
    for n, b in ((0, 0), (0, 2), (1, 1)):                    # their neighbours are untouched by it
        ref = R.hypothesis(x[n], sizes[n], "probs", hyps[n][b][0], hyps[n][b][1], space, frames=fr[n])
        _check_hyp(out, n, b, ref, True, "mean", "min", False)


def test_first_maximum_ties_and_nan_follow_the_greedy_scan():
    for C in (3, 70, 130):
        x = np.random.default_rng(C).random((1, 6, C)).astype(np.float32)
        x[0, 0, [1, C - 1]] = 2.0                            # a tie: the first wins
        x[0, 1, 0] = np.nan                                  # class 0 NaN: the scan never leaves it
        x[0, 2, 1] = np.nan                                  # a NaN elsewhere never wins
        x[0, 2, C - 1] = 3.0
        x[0, 3, :] = 0.25                                    # all equal
        x[0, 4, C - 1] = np.nan
        x[0, 4, C - 2] = 5.0
        x[0, 5, :] = -np.inf
        want = [R.argmax_first(x[0, t]) for t in range(6)]
        assert want == [1, 0, C - 1, 0, C - 2, 0]
        # every frame twice: a token of label want[t] on the first copy reaches the second one exactly when a_t is want[t] there
        x2 = np.repeat(x, 2, axis=1)
        out = _run(x2, [12], C, [[(want, list(range(0, 12, 2)))]], "probs", "max_prob", 1 / 3, "min", "min")
        assert out[0][0, 0].tolist() == list(range(0, 12, 2)) and out[1][0, 0].tolist() == list(range(1, 12, 2))
        assert _same_bits(out[2][0, 0], np.array([x[0, t, want[t]] for t in range(6)], np.float32))
        # ... and a token of any other label stays on its frame
        other = [(w + 1) % C for w in want]
        out = _run(x2, [12], C, [[(other, list(range(0, 12, 2)))]], "probs", "max_prob", 1 / 3, "min", "min")
        assert out[1][0, 0].tolist() == list(range(0, 12, 2))


def test_two_launches_give_identical_bits():
    z, sizes, space, hyps = _case(130, 65)
    for kind, measure in (("probs", "label_prob"), ("logits", "renyi"), ("log_probs", "entropy")):
        x = _x_of(z, kind)
        a = _run(x, sizes, space, hyps, kind, measure, 1 / 3, "mean", "min")
        b = _run(x, sizes, space, hyps, kind, measure, 1 / 3, "mean", "min")
        for u, v in zip(a, b):
            assert u.tobytes() == v.tobytes()


def test_limits_raise_value_errors_that_name_the_limit():
    from deepspeech.pytorch_amd import ops
    x = torch.zeros((1, 2, 3), device=DEV)
    tk = torch.zeros((1, 257, 2), dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match="at most 256 hypotheses"):
        ops.confidence(x, None, tk, tk, torch.zeros((1, 257), dtype=torch.int32, device=DEV), 0, 3)
    tk = tk[:, :1]
    ln = torch.zeros((1, 1), dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match="at most 8192 classes"):
        ops.confidence(torch.zeros((1, 2, 8193), device=DEV), None, tk, tk, ln, 0, 3)
    for kw in (dict(measure="tsallis", alpha=1.0), dict(alpha=0.0), dict(measure="margin"), dict(aggregate="max"), dict(kind="p")):
        with pytest.raises(ValueError):
            ops.confidence(x, None, tk, tk, ln, 0, 3, **kw)
    with pytest.raises(ValueError, match="2 classes"):
        ops.confidence(x[:, :, :1], None, tk, tk, ln, 0, 3, measure="entropy")


# ---- decoders ------------------------------------------------------------------------------------------------------------------
HOT = ["NEW YORK", ("TENT", 3.0)]


@functools.lru_cache(maxsize=None)
def _clips():
    p, sizes = HC.inputs(77, 3, 40, "toy3")
    return p, sizes


def _same_hypothesis(h, labels, offsets, x, size, space, conf, frame_seconds, exact, shift=0):
    """h against the reference applied to (labels, offsets) on the clip's frames x[:size]"""
    ref = R.hypothesis(x, size, "probs", labels, [o - shift for o in offsets], space, conf.measure, conf.alpha, conf.aggregate,
                       conf.word_aggregate)
    assert ref["valid"]
    assert h.labels == list(labels) and len(h.chars) == len(labels)
    assert [(c.start_frame - shift, c.end_frame - shift) for c in h.chars] == list(zip(ref["tok_start"], ref["tok_end"]))
    assert [w.text for w in h.words] == h.text.split() or space >= x.shape[1]
    assert [(w.start_frame - shift, w.end_frame - shift) for w in h.words] == [(w[2], w[3]) for w in ref["words"]]
    got = [c.confidence for c in h.chars] + [w.confidence for w in h.words] + ([h.confidence] if h.words else [])
    want = ref["tok_conf"] + [w[4] for w in ref["words"]] + ([ref["utt_conf"]] if h.words else [])
    if exact:
        assert _same_bits(got, want)
    else:
        assert np.allclose(np.array(got, np.float64), np.array(want, np.float64), rtol=0, atol=2 * U)
    assert (h.confidence is None) == (not ref["words"])
    for s in h.chars + h.words:
        if frame_seconds is None:
            assert s.start_s is None and s.end_s is None
        else:
            assert s.start_s == s.start_frame * frame_seconds and s.end_s == (s.end_frame + 1) * frame_seconds


def _confs():
    from deepspeech.pytorch_amd.confidence import Confidence
    return [(None, True), (Confidence("max_prob", aggregate="prod", word_aggregate="mean"), True),
            (Confidence("entropy", aggregate="min", word_aggregate="mean"), False)]


def test_greedy_decode_words_equals_the_reference_on_decode():
    from deepspeech.pytorch_amd.confidence import Confidence
    from deepspeech.pytorch_amd.decoder import GreedyDecoder
    p, sizes = _clips()
    lab = HC.labels()
    dec = GreedyDecoder(lab)
    pd, sz = torch.from_numpy(p).to(DEV), torch.from_numpy(sizes)
    strings, offsets = dec.decode(pd, sz)
    for conf, exact in _confs():
        hyps = dec.decode_words(pd, sz, confidence=conf, frame_seconds=0.02)
        assert len(hyps) == 3 and hyps[1].text == "" and hyps[1].confidence is None and hyps[1].words == []
        for n, h in enumerate(hyps):
            assert h.text == strings[n][0] and h.score is None and h.acoustic is None
            _same_hypothesis(h, [lab.index(c) for c in h.text], offsets[n][0].tolist(), p[n], int(sizes[n]), dec.space_index,
                             conf or Confidence(), 0.02, exact)
    assert any(len(h.words) > 1 for h in hyps)
    # the span of a greedy character is its arg-max run
    a = p[0].argmax(-1)
    for c in hyps[0].chars:
        l = lab.index(c.text)
        assert (a[c.start_frame:c.end_frame + 1] == l).all()
        assert c.start_frame == 0 or a[c.start_frame - 1] != l
        assert c.end_frame + 1 == sizes[0] or a[c.end_frame + 1] != l


@pytest.mark.parametrize("form", ["plain", "hot", "lm", "lm_hot"])
@pytest.mark.parametrize("nbest", [1, 8])
def test_beam_decode_words_equals_the_reference_on_decode_beams(form, nbest):
    from deepspeech.pytorch_amd.confidence import Confidence
    from deepspeech.pytorch_amd.decoder import BeamCTCDecoder
    p, sizes = _clips()
    lab = HC.labels()
    arpa = os.path.join(HC.GOLDEN, "toy3.arpa")
    dec = BeamCTCDecoder(lab, lm_path=arpa if "lm" in form else None, alpha=1.2, beta=0.8, beam_width=8,
                         hotwords=HOT if "hot" in form else None)
    pd, sz = torch.from_numpy(p).to(DEV), torch.from_numpy(sizes)
    strings, offsets, scores, acoustic = dec.decode_beams_detailed(pd, sz)
    for conf, exact in _confs()[::2]:
        out = dec.decode_words(pd, sz, confidence=conf, nbest=nbest)
        assert len(out) == 3 and all(len(o) == nbest for o in out)
        for n in range(3):
            for r, h in enumerate(out[n]):
                assert h.text == strings[n][r]
                assert np.float32(h.score).tobytes() == scores[n, r].numpy().tobytes()
                assert np.float32(h.acoustic).tobytes() == acoustic[n, r].numpy().tobytes()
                _same_hypothesis(h, [lab.index(c) for c in h.text], offsets[n][r].tolist(), p[n], int(sizes[n]), dec.space_index,
                                 conf or Confidence(), None, exact)
    assert any(len(h.words) > 1 for o in out for h in o)


def test_decode_words_without_frames():
    from deepspeech.pytorch_amd.decoder import BeamCTCDecoder, GreedyDecoder
    lab = HC.labels()
    p = torch.zeros((2, 0, len(lab)), device=DEV)
    assert [h.text for h in GreedyDecoder(lab).decode_words(p)] == ["", ""]
    out = BeamCTCDecoder(lab, beam_width=4).decode_words(p, nbest=2)
    assert [[h.text for h in o] for o in out] == [["", ""], ["", ""]] and out[0][0].score == 0.0 and out[0][1].score == float("inf")


# ---- streams -------------------------------------------------------------------------------------------------------------------
def _hyp_key(h, shift=0):
    """everything of a Hypothesis, the floats as bits; shift is added to its frames"""
    f = lambda v: None if v is None else np.float32(v).tobytes()
    return (h.text, f(h.score), f(h.acoustic), f(h.confidence), tuple(h.labels),
            tuple((s.text, s.start_frame + shift, s.end_frame + shift, f(s.confidence), s.start_s, s.end_s) for s in h.chars + h.words))


@functools.lru_cache(maxsize=None)
def _stream_clips():
    p, _ = HC.inputs(78, 2, 60, "toy3")
    return p


# chunk sizes of (stream 0, stream 1): a feed of nothing for one stream, a one-frame chunk, uneven chunks
CHUNKINGS = [[(60, 60)], [(1, 0), (0, 7), (29, 23), (30, 30)], [(13, 1), (1, 13), (0, 0), (46, 46)]]


@pytest.mark.parametrize("form", ["plain", "lm_hot"])
@pytest.mark.parametrize("chunks", CHUNKINGS, ids=["whole", "ragged", "late"])
def test_beam_stream_words_equal_decode_words_after_every_feed(form, chunks):
    from deepspeech.pytorch_amd.confidence import Confidence
    from deepspeech.pytorch_amd.decoder import BeamCTCDecoder
    p, lab = _stream_clips(), HC.labels()
    dec = BeamCTCDecoder(lab, lm_path=os.path.join(HC.GOLDEN, "toy3.arpa") if form == "lm_hot" else None, alpha=1.2, beta=0.8,
                         beam_width=8, hotwords=HOT if form == "lm_hot" else None)
    conf = Confidence("max_prob", aggregate="mean", word_aggregate="prod")
    st = dec.stream(2, 60, DEV, confidence=conf)
    pd = torch.from_numpy(p).to(DEV)
    pos = [0, 0]
    for sizes in chunks:
        Tc = max(max(sizes), 1)
        x = torch.zeros((2, Tc, len(lab)), device=DEV)
        for n in range(2):
            x[n, :sizes[n]] = pd[n, pos[n]:pos[n] + sizes[n]]
        st.feed(x, list(sizes))
        pos = [a + b for a, b in zip(pos, sizes)]
        assert st.frames == pos
        for nbest in (1, 8):
            got = st.words(nbest, frame_seconds=0.02)
            for n in range(2):
                want = dec.decode_words(pd[n:n + 1, :max(pos[n], 1)], torch.tensor([pos[n]]), conf, nbest, 0.02)[0]
                assert [_hyp_key(h) for h in got[n]] == [_hyp_key(h) for h in want], (sizes, n, nbest)
        assert [_hyp_key(h) for h in st.best_words(0.02)] == [_hyp_key(g[0]) for g in got]
    assert pos == [60, 60] and any(len(h.words) > 1 for h in st.best_words())
    with pytest.raises(ValueError, match="max_frames"):
        st.feed(pd[:, :1], [1, 0])
    st.reset([1])
    st.feed(pd[:, :5].contiguous(), [0, 5])
    got = st.best_words()
    assert _hyp_key(got[1]) == _hyp_key(dec.decode_words(pd[1:, :5], None, conf)[0][0])
    assert _hyp_key(got[0]) == _hyp_key(dec.decode_words(pd[:1], None, conf)[0][0])


@pytest.mark.parametrize("chunks", CHUNKINGS, ids=["whole", "ragged", "late"])
def test_greedy_stream_words_equal_decode_words_and_need_max_frames(chunks):
    from deepspeech.pytorch_amd.confidence import Confidence
    from deepspeech.pytorch_amd.decoder import GreedyDecoder
    p, lab = _stream_clips(), HC.labels()
    dec, conf = GreedyDecoder(lab), Confidence()
    with pytest.raises(ValueError, match="max_frames"):
        dec.stream(2, DEV, confidence=conf)
    st = dec.stream(2, DEV, confidence=conf, max_frames=60)
    pd = torch.from_numpy(p).to(DEV)
    pos = [0, 0]
    for sizes in chunks:
        Tc = max(max(sizes), 1)
        x = torch.zeros((2, Tc, len(lab)), device=DEV)
        for n in range(2):
            x[n, :sizes[n]] = pd[n, pos[n]:pos[n] + sizes[n]]
        st.feed(x, list(sizes))
        pos = [a + b for a, b in zip(pos, sizes)]
        got = st.words(frame_seconds=0.02)
        for n in range(2):
            want = dec.decode_words(pd[n:n + 1, :max(pos[n], 1)], torch.tensor([pos[n]]), conf, 0.02)[0]
            assert _hyp_key(got[n]) == _hyp_key(want) and got[n].text == st.text[n]
    with pytest.raises(ValueError, match="max_frames"):
        st.feed(pd[:, :1], [0, 1])


def test_streams_without_confidence_keep_no_frames():
    from deepspeech.pytorch_amd.confidence import Confidence
    from deepspeech.pytorch_amd.decoder import BeamCTCDecoder, Endpointer, GreedyDecoder
    lab = HC.labels()
    b, ep = BeamCTCDecoder(lab, beam_width=4), Endpointer(min_trailing=3, max_leading=5, max_segment=10)
    for st in (b.stream(2, 20, DEV), b.stream(2, 20, DEV, endpoint=ep), GreedyDecoder(lab).stream(2, DEV),
               GreedyDecoder(lab).stream(2, DEV, endpoint=ep)):
        assert st._store is None and st.confidence is None
        with pytest.raises(ValueError, match="confidence="):
            st.words()
    assert b.stream(2, 20, DEV, confidence=Confidence())._store.rows.shape == (2, 20, len(lab))


def test_frame_store_wraps_and_reads_sizes_on_the_device():
    from deepspeech.pytorch_amd import ops
    rng = np.random.default_rng(5)
    st = ops.frame_store_open(3, 7, 5, DEV)
    want = [np.zeros((0, 5), np.float32) for _ in range(3)]
    for sizes in ([3, 0, 5], [4, 1, 5], [0, 0, 0], [7, 2, 1], [9, 9, 3]):          # the last chunk is longer than the store
        Tc = max(max(sizes), 1)
        x = rng.random((3, Tc, 5)).astype(np.float32)
        ops.frame_store_append(st, torch.from_numpy(x).to(DEV), torch.tensor(sizes, dtype=torch.int32, device=DEV))
        want = [np.concatenate([w, x[n, :sizes[n]]]) for n, w in enumerate(want)]
    rows, count = st.rows.cpu().numpy(), st.count.cpu().tolist()
    assert count == [len(w) for w in want] == [23, 12, 14]
    for n in range(3):
        for f in range(max(0, count[n] - 7), count[n]):
            assert (rows[n, f % 7] == want[n][f]).all()
    x = torch.from_numpy(rng.random((3, 2, 5)).astype(np.float32)).to(DEV)
    ops.frame_store_append(st, x)                                                # sizes None: the whole chunk
    assert st.count.cpu().tolist() == [25, 14, 16] and torch.equal(st.rows[0, 24 % 7], x[0, 1])
    ops.frame_store_reset(st, [1])
    assert st.count.cpu().tolist() == [25, 0, 16]


def test_ring_addressed_frames_give_the_same_words():
    """ops.confidence on a ring: hypothesis row n reads frame t at row (t0[n] + t) % cap"""
    from deepspeech.pytorch_amd import ops
    z, sizes, space, hyps = _case(64, 29)
    x = _x_of(z, "probs")
    flat = _run(x, sizes, space, hyps, "probs", "label_prob", 1 / 3, "mean", "min")
    t0 = [5, 63, 0]
    ring = np.stack([np.roll(x[n], t0[n], axis=0) for n in range(3)])
    N, B = 3, 3
    ld = max(1, max(len(h[0]) for hs in hyps for h in hs))
    tok, off, lens = np.zeros((N, B, ld), np.int32), np.zeros((N, B, ld), np.int32), np.zeros((N, B), np.int32)
    for n in range(N):
        for b in range(B):
            t, o = hyps[n][b]
            tok[n, b, :len(t)], off[n, b, :len(o)], lens[n, b] = t, o, len(t)
    out = ops.confidence(torch.from_numpy(ring).to(DEV), torch.tensor(sizes, dtype=torch.int32), torch.from_numpy(tok).to(DEV),
                         torch.from_numpy(off).to(DEV), torch.from_numpy(lens).to(DEV), 0, space,
                         t0=torch.tensor(t0, dtype=torch.int32), cap=64)
    for u, v in zip(flat, out):
        assert u.tobytes() == v.cpu().numpy().tobytes()


def _session_case():
    """the tiny uni-directional fixture model on 160 synthetic frames of 2 streams, fed in chunks of which the first is exactly
    the model's latency and the second a single frame"""
    from deepspeech.pytorch_amd import synth
    from fixtures import Fixture
    from test_gpu_model import build
    fx, lengths = Fixture("gru_uni_la"), [160, 155]
    x = torch.from_numpy(synth.synth_batch(np.asarray(lengths), seed=11)[0]).to(DEV)
    return fx, build(fx, 32).eval(), x, lengths, [54, 1, 2, 37, 66]


@pytest.mark.parametrize("kind", ["greedy", "beam"])
def test_streaming_transcriber_words_equal_decode_words_on_its_probabilities(kind):
    from deepspeech.pytorch_amd import decoder as D
    from deepspeech.pytorch_amd.confidence import Confidence
    from deepspeech.pytorch_amd.streaming import StreamingTranscriber
    fx, m, x, lengths, chunks = _session_case()
    dec = D.GreedyDecoder(fx.labels) if kind == "greedy" else D.BeamCTCDecoder(fx.labels, beam_width=8)
    conf = Confidence()
    st = StreamingTranscriber(m, dec, carry_context=True, max_frames=80, confidence=conf)
    assert st.words() == []
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
        want = dec.decode_words(pn, None, conf)[0]
        assert [_hyp_key(h) for h in got[n]] == [_hyp_key(h) for h in (want if kind == "beam" else [want])]
    assert [_hyp_key(h) for h in st.best_words()] == [_hyp_key(g[0]) for g in got]


def test_stream_pool_words_of_staggered_slots_equal_decode_words():
    from deepspeech.pytorch_amd import decoder as D
    from deepspeech.pytorch_amd.confidence import Confidence
    from deepspeech.pytorch_amd.streaming import StreamPool
    fx, m, x, lengths, chunks = _session_case()
    dec, conf = D.BeamCTCDecoder(fx.labels, beam_width=8), Confidence("entropy")
    pool = StreamPool(m, dec, 2, max_frames=80, confidence=conf)
    slot, fed, outs = {}, [0, 0], [[], []]
    tick = 0
    while any(f < g for f, g in zip(fed, lengths[:2])):
        if tick < 2:
            slot[tick] = pool.open()                         # the second slot opens one tick after the first
            assert pool.words(slot[tick])[0].text == ""
        rows = [k for k in slot if fed[k] < lengths[k]]
        lens = [min(chunks[tick % len(chunks)], lengths[k] - fed[k]) for k in rows]
        final = [k for k, c in zip(rows, lens) if fed[k] + c == lengths[k]]
        xc = torch.zeros((len(rows), 1, x.shape[2], max(lens)), device=DEV)
        for r, k in enumerate(rows):
            xc[r, :, :, :lens[r]] = x[k, :, :, fed[k]:fed[k] + lens[r]]
        pool.feed([slot[k] for k in rows], xc, lens, final=[slot[k] for k in final])
        for r, k in enumerate(rows):
            if pool.last_output.get(slot[k]) is not None:
                outs[k].append(pool.last_output[slot[k]])
            fed[k] += lens[r]
        tick += 1
    for k in range(2):
        pk = torch.cat(outs[k])[None]
        assert pk.shape[1] == pool.frames(slot[k]) > 0
        want = dec.decode_words(pk, None, conf, nbest=2)[0]
        assert [_hyp_key(h) for h in pool.words(slot[k], nbest=2)] == [_hyp_key(h) for h in want]


# ---- endpointed streams: the frames live in a ring ------------------------------------------------------------------------------
EP_CHUNKS = [(37, 30), (1, 0), (0, 25), (62, 45)]          # 100 frames per stream, in sub-feeds of sub_feed = 3 frames


@functools.lru_cache(maxsize=None)
def _endpoint_clips():
    """2 x 100 frames of planted sentences with pauses: runs of 1 to 6 frames whose blank probability is 0.97"""
    p, _ = HC.inputs(79, 2, 100, "toy3")
    p = p.copy()
    rng = np.random.default_rng(7)
    for n in range(2):
        t = int(rng.integers(0, 6))
        while t < 100:
            run = int(rng.integers(1, 7))
            p[n, t:t + run] = 0.03 / (p.shape[2] - 1)
            p[n, t:t + run, 0] = 0.97
            t += run + int(rng.integers(2, 12))
    return p


def _endpointer():
    from deepspeech.pytorch_amd.decoder import Endpointer
    return Endpointer(blank_threshold=0.8, min_trailing=3, max_leading=5, max_segment=8)


def _same_segment(a, b):
    from deepspeech.pytorch_amd.decoder import Segment
    assert isinstance(a, Segment) and a._fields == Segment._fields and len(a) == len(b) == 9
    assert (a.index, a.start, a.end, a.reason, a.strings, a.labels) == (b.index, b.start, b.end, b.reason, b.strings, b.labels)
    assert all(torch.equal(u, v) for u, v in zip(a.offsets, b.offsets))
    for u, v in ((a.scores, b.scores), (a.acoustic, b.acoustic)):
        assert (u is None and v is None) or torch.equal(u, v)


def _run_endpointed(dec, open_stream, want_segment, want_open):
    """feeds EP_CHUNKS to a stream with confidence= and to one without; checks every finished segment and, after every feed,
    the open segment's partial; returns the segments per stream"""
    from deepspeech.pytorch_amd import ops
    from deepspeech.pytorch_amd.decoder import WordSegment
    p = _endpoint_clips()
    pd = torch.from_numpy(p).to(DEV)
    st, plain = open_stream(True), open_stream(False)
    assert plain._store is None and st._store.rows.shape[1] == 8 + 8 * 3
    pos, got, ref = [0, 0], [[], []], [[], []]
    for step, sizes in enumerate(EP_CHUNKS + [None]):
        if sizes is None:
            st.end(), plain.end()
        else:
            x = torch.zeros((2, max(sizes), p.shape[2]), device=DEV)
            for n in range(2):
                x[n, :sizes[n]] = pd[n, pos[n]:pos[n] + sizes[n]]
            st.feed(x, list(sizes)), plain.feed(x, list(sizes))
            pos = [a + b for a, b in zip(pos, sizes)]
            starts = ops.endpoint_state(st._ep)[:, 0].tolist()
            want_open(st, pd, starts, pos)
        for n, (a, b) in enumerate(zip(st.segments(), plain.segments())):
            got[n] += a
            ref[n] += b
    for n in range(2):
        assert len(got[n]) == len(ref[n]) > 8                # more than RING_SLOTS segments, and the 32-frame ring wrapped thrice
        assert got[n][-1].reason == "final" and got[n][-1].end == 99
        for a, b in zip(got[n], ref[n]):
            assert isinstance(a, WordSegment) and not isinstance(b, WordSegment)
            _same_segment(a, b)
            want_segment(a, pd[n:n + 1, a.start:a.end + 1])
            assert a.confidence == a.hypotheses[0].confidence
    assert any(len(h.words) > 0 for segs in got for s in segs for h in s.hypotheses)
    return got


@pytest.mark.parametrize("form", ["plain", "lm_hot"])
def test_endpointed_beam_stream_segments_carry_decode_words_of_their_frames(form):
    from deepspeech.pytorch_amd.confidence import Confidence
    from deepspeech.pytorch_amd.decoder import BeamCTCDecoder
    lab = HC.labels()
    dec = BeamCTCDecoder(lab, lm_path=os.path.join(HC.GOLDEN, "toy3.arpa") if form == "lm_hot" else None, alpha=1.2, beta=0.8,
                         beam_width=8, hotwords=HOT if form == "lm_hot" else None)
    conf = Confidence("max_prob", aggregate="mean", word_aggregate="prod")

    def want_segment(seg, frames):
        want = dec.decode_words(frames, None, conf, nbest=2)[0]
        assert [_hyp_key(h) for h in seg.hypotheses] == [_hyp_key(h, seg.start) for h in want]

    def want_open(st, pd, starts, pos):
        got = st.words(2)
        for n in range(2):
            want = dec.decode_words(pd[n:n + 1, starts[n]:max(pos[n], starts[n] + 1)], torch.tensor([pos[n] - starts[n]]), conf, 2)[0]
            assert [_hyp_key(h) for h in got[n]] == [_hyp_key(h, starts[n]) for h in want]
        assert [_hyp_key(h) for h in st.best_words()] == [_hyp_key(g[0]) for g in got]

    _run_endpointed(dec, lambda c: dec.stream(2, 16, DEV, endpoint=_endpointer(), nbest=2, confidence=conf if c else None),
                    want_segment, want_open)


def test_endpointed_greedy_stream_segments_carry_decode_words_of_their_frames():
    from deepspeech.pytorch_amd.confidence import Confidence
    from deepspeech.pytorch_amd.decoder import GreedyDecoder
    dec, conf = GreedyDecoder(HC.labels()), Confidence("entropy", aggregate="min", word_aggregate="mean")

    def want_segment(seg, frames):
        assert len(seg.hypotheses) == 1
        assert _hyp_key(seg.hypotheses[0]) == _hyp_key(dec.decode_words(frames, None, conf)[0], seg.start)

    def want_open(st, pd, starts, pos):
        got = st.best_words()
        for n in range(2):
            want = dec.decode_words(pd[n:n + 1, starts[n]:max(pos[n], starts[n] + 1)], torch.tensor([pos[n] - starts[n]]), conf)[0]
            assert _hyp_key(got[n]) == _hyp_key(want, starts[n]) and got[n].text == st.text[n]

    _run_endpointed(dec, lambda c: dec.stream(2, DEV, endpoint=_endpointer(), confidence=conf if c else None),
                    want_segment, want_open)


def test_sessions_with_endpoint_and_confidence_return_word_segments():
    from deepspeech.pytorch_amd import decoder as D
    from deepspeech.pytorch_amd.confidence import Confidence
    from deepspeech.pytorch_amd.streaming import StreamingTranscriber, StreamPool
    fx, m, x, lengths, chunks = _session_case()
    dec, conf = D.BeamCTCDecoder(fx.labels, beam_width=8), Confidence()
    st = StreamingTranscriber(m, dec, carry_context=True, max_frames=16, endpoint=_endpointer(), confidence=conf)
    pool = StreamPool(m, dec, 2, max_frames=16, endpoint=_endpointer(), confidence=conf)
    slots = [pool.open(), pool.open()]
    assert [h.score for h in pool.words(slots[0], nbest=2)] == [0.0, float("inf")]          # decode_words on no frames
    pos, outs = 0, [[] for _ in lengths]
    for i, c in enumerate(chunks):
        last = i == len(chunks) - 1
        lens = [g - pos for g in lengths] if last else [c] * len(lengths)
        xc = x[:, :, :, pos:pos + c].contiguous()
        st.feed(xc, lens, final=last)
        pool.feed(slots, xc, lens, final=slots if last else ())
        if st.last_output is not None:
            probs, sizes = st.last_output
            for n in range(len(lengths)):
                outs[n].append(probs[n, :int(sizes[n])])
        pos += c
    segs = st.segments()
    for n in range(len(lengths)):
        pn, psegs = torch.cat(outs[n])[None], pool.segments(slots[n])
        assert len(segs[n]) == len(psegs) > 2
        for a, b in zip(segs[n], psegs):
            assert isinstance(a, D.WordSegment) and isinstance(b, D.WordSegment)
            want = dec.decode_words(pn[:, a.start:a.end + 1], None, conf)[0]
            assert [_hyp_key(h) for h in a.hypotheses] == [_hyp_key(h, a.start) for h in want]
            assert [_hyp_key(h) for h in b.hypotheses] == [_hyp_key(h) for h in a.hypotheses]
