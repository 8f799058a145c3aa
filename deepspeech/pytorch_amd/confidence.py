"""Word timings and confidence for what the CTC decoders return.

``decoder.decode_words(probs, sizes, confidence=Confidence(...))`` gives, per clip, ``Hypothesis`` tuples whose ``words`` and
``chars`` carry their first and last frame (inclusive), seconds when the frame duration is known, and a confidence in [0, 1].
The spans and the confidences are computed on the device (ds2_confidence: one frame pass, one wave per hypothesis; the rules
are in include/ds2hip.h and DESIGN.md section 3.8) from the decode's own device buffers; the tuples below, the argument checks
and the seconds conversion are host bookkeeping and import without a GPU.

The measures are DEFINED here, not validated: nothing in this project says how well any of them predicts that a word is
right on any corpus.  Calibration is the caller's business.
"""
import contextlib
import gc
import itertools
from collections import namedtuple

_NONE = itertools.repeat(None)
MEASURES = {"label_prob": 0, "max_prob": 1, "entropy": 2, "tsallis": 3, "renyi": 4}
AGGREGATES = {"mean": 0, "min": 1, "prod": 2}

# frames are inclusive; start_s / end_s are None unless the frame duration is known (start_frame * frame_seconds and
# (end_frame + 1) * frame_seconds, as align.make_span); confidence is a float
Word = namedtuple("Word", "text start_frame end_frame confidence start_s end_s")
Char = namedtuple("Char", "text start_frame end_frame confidence start_s end_s")
# score / acoustic: decode_beams_detailed's values of the same rank (None for a greedy decode); confidence: None without words;
# labels: the hypothesis as label indices
Hypothesis = namedtuple("Hypothesis", "text score acoustic confidence words chars labels")


class Confidence:
    """What a token's, a word's and an utterance's confidence is.  measure: the per-frame value --
    "label_prob" (the probability of the token's own label), "max_prob" (of the frame's arg-max), or 1 - normalised "entropy" /
    "tsallis" / "renyi" entropy of the frame's distribution (the latter two of order alpha).  aggregate: how a token combines the
    frames of its span, word_aggregate: how a word combines its tokens and an utterance its words; each "mean", "min" or "prod".
    The defaults are the conventional choices (mean label probability per token, the weakest token per word, entropy order
    1/3), not tuned on any data."""

    def __init__(self, measure="label_prob", alpha=1 / 3, aggregate="mean", word_aggregate="min"):
        if measure not in MEASURES:
            raise ValueError("measure must be one of %s, got %r" % (sorted(MEASURES), measure))
        for name, v in (("aggregate", aggregate), ("word_aggregate", word_aggregate)):
            if v not in AGGREGATES:
                raise ValueError("%s must be one of %s, got %r" % (name, sorted(AGGREGATES), v))
        alpha = float(alpha)
        if not alpha > 0 or alpha == float("inf"):
            raise ValueError("alpha must be a positive finite number, got %r" % (alpha,))
        if alpha == 1 and measure in ("tsallis", "renyi"):
            raise ValueError("alpha == 1 is the Shannon limit: use measure='entropy' instead of %r" % (measure,))
        self.measure, self.alpha, self.aggregate, self.word_aggregate = measure, alpha, aggregate, word_aggregate

    def check_classes(self, num_classes):
        if MEASURES[self.measure] >= MEASURES["entropy"] and num_classes < 2:
            raise ValueError("measure %r needs at least 2 classes, got %d" % (self.measure, num_classes))

    def codes(self):
        """(measure, alpha, aggregate, word_aggregate) as ds2_confidence takes them"""
        return MEASURES[self.measure], self.alpha, AGGREGATES[self.aggregate], AGGREGATES[self.word_aggregate]

    def __repr__(self):
        return "Confidence(measure=%r, alpha=%r, aggregate=%r, word_aggregate=%r)" % (
            self.measure, self.alpha, self.aggregate, self.word_aggregate)


@contextlib.contextmanager
def building_tuples():
    """Around the loop that builds the Char / Word tuples, and nothing else: everything alive before it is moved to the permanent
    generation (gc.freeze), so the collections that millions of new tuples trigger walk only those tuples' generation and not
    the process' whole heap, and is moved back afterwards.  The collector stays ON, for this thread and every other.  (The
    tuples hold strings and numbers only; unfrozen, the collections took 3/4 of the host time of decode_words at nbest =
    beam_width = 128.)"""
    gc.freeze()
    try:
        yield
    finally:
        gc.unfreeze()


def _seconds(start, end, frame_seconds):
    if frame_seconds is None:
        return None, None
    return int(start) * frame_seconds, (int(end) + 1) * frame_seconds


def make_hypothesis(labels, int_to_char, space_index, res, score=None, acoustic=None, frame_seconds=None, shift=0):
    """One Hypothesis from a hypothesis' labels and its rows of ds2_confidence's outputs as host lists: res = (tok_start, tok_end,
    tok_conf, word_first, word_last, word_start, word_end, word_conf, word_count, utt_conf).  shift is added to every frame (a
    segment's start in its stream).  An invalid hypothesis (no spans) comes back without chars and words."""
    ts, te, tc, wf, wl, ws, we, wc, count, utt = res
    text = ''.join(' ' if v == space_index else int_to_char[v] for v in labels)
    chars, words = [], []
    if len(labels) == 0 or ts[0] >= 0:
        if shift:
            ts, te = [v + shift for v in ts], [v + shift for v in te]
        if frame_seconds is None:       # the tuples are the host's whole cost at large nbest: no Python-level call per character
            chars = list(map(Char._make, zip(text, ts, te, tc, _NONE, _NONE)))
        else:
            chars = list(map(Char._make, zip(text, ts, te, tc, [v * frame_seconds for v in ts],
                                             [(v + 1) * frame_seconds for v in te])))
        for w in range(int(count)):
            s, e = ws[w] + shift, we[w] + shift
            words.append(Word(text[wf[w]:wl[w] + 1], s, e, float(wc[w]), *_seconds(s, e, frame_seconds)))
    return Hypothesis(text, score, acoustic, float(utt) if words else None, words, chars, list(labels))
