"""Keyword spotting on the CTC outputs: was one of these phrases said, and where -- without a decode.

``KeywordSpotter(labels, ["hey there", ("stop", -0.5)]).spot(out, sizes)`` runs, for every keyword, the CTC max-lattice over the
keyword's labels with a free start and a free end through the network's outputs on the device (ds2_kws_feed; the rule is stated
in include/ds2hip.h and DESIGN.md section 3.9) and returns one list of ``Detection`` per clip.  A detection's score is a
log-likelihood ratio in nats: the best path through the keyword on its frames against the greedy path on the same frames, 0
exactly when the greedy path spells the keyword there and negative otherwise.  ``spotter.stream(n, device)`` is the same for
``n`` endless streams fed chunk by chunk: the lattice, the open candidate and the best score of every (stream, keyword) stay on the
device between the feeds, and the hits are the one-shot call's whatever the chunking.

A keyword is a string over the labels; the space label may stand anywhere in it, also first or last, which is how a caller
asks for a word boundary (" stop " does not fire inside "unstoppable").

The lattice runs on the device; the string-to-label mapping, the packing of the keywords into waves and the tuples below are
host bookkeeping and import without a GPU (ops, and with it the HIP library, is imported on the first call).

The defaults (threshold -1.0 nats per label, hold 25 frames) are DEFINED here, not calibrated: nothing in this project says
which threshold separates hits from false alarms on any corpus.  ``return_best`` / ``best()`` give the largest score of every
keyword whatever the threshold, from which a caller calibrates one.
"""
import warnings
from collections import namedtuple

import numpy as np
import torch

KINDS = {"logits": 0, "probs": 1, "log_probs": 2}
MAX_LABELS = 64                       # labels of one keyword: one wave
MAX_HITS = 4096                       # ds2_kws_feed's bound on max_hits
FIRST, LAST, SKIP = 1, 2, 4           # lane flags of the packing (csrc/ds2_kws.hip names the same bits)

# frames are inclusive and absolute (counted from the start of the clip or stream); score is in nats, <= 0; score_per_label =
# score / labels of the keyword, what `threshold` is compared with; start_s / end_s are None unless the frame duration is known
# (start_frame * frame_seconds and (end_frame + 1) * frame_seconds, as align.make_span); index is the keyword's position in the list
Detection = namedtuple("Detection", "keyword index start_frame end_frame score score_per_label start_s end_s")
# best(): per keyword the largest end score so far and its span; score -inf and frames -1 before any path exists
Best = namedtuple("Best", "keyword index start_frame end_frame score score_per_label")


def normalize(keywords, default_threshold):
    """[(keyword, threshold as a Python float), ...] from a list of strings or (string, threshold) pairs."""
    out = []
    for item in keywords or []:
        if isinstance(item, str):
            kw, thr = item, default_threshold
        else:
            try:
                kw, thr = item
            except (TypeError, ValueError):
                raise ValueError("a keyword is a string or a (string, threshold) pair, got %r" % (item,))
            if not isinstance(kw, str):
                raise ValueError("a keyword is a string or a (string, threshold) pair, got %r" % (item,))
        try:
            thr = float(thr)
        except (TypeError, ValueError):
            raise ValueError("keyword %r: the threshold %r is no number" % (kw, thr))
        if thr != thr or thr > 0 or thr == float("-inf"):
            raise ValueError("keyword %r: the threshold is a finite number of nats per label <= 0, got %r" % (kw, thr))
        out.append((kw, thr))
    if not out:
        raise ValueError("a keyword spotter needs at least one keyword")
    return out


def keyword_labels(keyword, labels, blank):
    """The label ids of a keyword; ValueError (naming the keyword) when it breaks a rule."""
    if not keyword:
        raise ValueError("keyword %r is empty" % keyword)
    index = {c: i for i, c in enumerate(labels) if i != blank}
    ids = []
    for ch in keyword:
        if ch not in index:
            raise ValueError("keyword %r contains %r, which is the blank or no label" % (keyword, ch))
        ids.append(index[ch])
    if len(ids) > MAX_LABELS:
        raise ValueError("keyword %r has %d labels; a keyword takes 1 to %d" % (keyword, len(ids), MAX_LABELS))
    return tuple(ids)


def threshold_abs(threshold, num_labels):
    """thr_abs = fp32(threshold * L): the product in fp64, rounded once"""
    return np.float32(np.float64(threshold) * num_labels)


def pack_waves(lengths):
    """The packing rule: the keywords fill waves of 64 lanes in list order, one lane per label; a keyword that does not fit into
    what is left of the current wave starts the next one, so none straddles a wave.  Returns [(wave, first lane)] per keyword
    and the number of waves."""
    where, wave, used = [], 0, 0
    for L in lengths:
        if not 1 <= L <= MAX_LABELS:
            raise ValueError("a keyword takes 1 to %d labels, got %d" % (MAX_LABELS, L))
        if used + L > 64:
            wave, used = wave + 1, 0
        where.append((wave, used))
        used += L
    return where, wave + 1


def pack(label_ids, thresholds):
    """The lane table ds2_kws_feed takes: int32 (waves * 64, 4) of (label, flags, keyword index, thr_abs bits); an unused lane
    is (-1, 0, -1, 0).  flags: FIRST on a keyword's first label, LAST on its last, SKIP where y_i != y_{i-1}."""
    where, waves = pack_waves([len(ids) for ids in label_ids])
    lanes = np.zeros((waves * 64, 4), np.int32)
    lanes[:, 0] = -1
    lanes[:, 2] = -1
    for k, (ids, thr, (w, l0)) in enumerate(zip(label_ids, thresholds, where)):
        bits = int(np.float32(threshold_abs(thr, len(ids))).view(np.int32))
        for i, y in enumerate(ids):
            flags = (FIRST if i == 0 else 0) | (LAST if i == len(ids) - 1 else 0) | (SKIP if i > 0 and y != ids[i - 1] else 0)
            lanes[w * 64 + l0 + i] = (y, flags, k, bits)
    return lanes


class KeywordSpotter:
    """keywords: a list of strings or (string, threshold) pairs over `labels`.  threshold: nats per label, <= 0: a keyword of L
    labels fires where its end score reaches fp32(threshold * L).  hold: frames (>= 1) an open candidate waits for a better end
    before it is emitted; overlapping ends of one occurrence merge within it.  max_hits: the hits of one keyword that one feed
    (or one ``spot`` call) keeps per clip or stream; the others are counted (``dropped``) and not returned.
    The defaults are defined, not calibrated on any data (module docstring)."""

    def __init__(self, labels, keywords, threshold=-1.0, hold=25, blank_index=0, frame_seconds=None, max_hits=8):
        self.labels, self.blank_index, self.frame_seconds = labels, int(blank_index), frame_seconds
        if not 0 <= self.blank_index < len(labels):
            raise ValueError("blank index %d out of range for %d labels" % (blank_index, len(labels)))
        if int(hold) != hold or int(hold) < 1:
            raise ValueError("hold must be a frame count >= 1, got %r" % (hold,))
        if int(max_hits) != max_hits or not 1 <= int(max_hits) <= MAX_HITS:
            raise ValueError("max_hits must be in [1, %d], got %r" % (MAX_HITS, max_hits))
        self.hold, self.max_hits = int(hold), int(max_hits)
        items = normalize(keywords, threshold)
        seen = {}
        self.keywords, self.thresholds, self.label_ids = [], [], []
        for kw, thr in items:
            ids = keyword_labels(kw, labels, self.blank_index)
            if ids in seen:
                raise ValueError("keyword %r is listed twice" % kw)
            seen[ids] = kw
            self.keywords.append(kw)
            self.thresholds.append(thr)
            self.label_ids.append(ids)
        self.lanes = pack(self.label_ids, self.thresholds)
        self.last_dropped = []                         # per clip of the last spot(): the hits beyond max_hits per keyword

    @classmethod
    def from_model(cls, model, keywords, **kw):
        """The spotter of a DeepSpeech model: its labels and blank, and the duration of one output frame (the conv stack's time
        stride is 2, so a frame is two spectrogram hops), as ForcedAligner.from_model."""
        return cls(model.labels, keywords, blank_index=model.blank_index, frame_seconds=2 * model.spect_cfg.window_stride, **kw)

    def detection(self, k, start, end, score):
        fs = self.frame_seconds
        return Detection(self.keywords[k], k, int(start), int(end), float(score), float(score) / len(self.label_ids[k]),
                         None if fs is None else int(start) * fs, None if fs is None else (int(end) + 1) * fs)

    def detections(self, hits):
        """One stream's device hits as Detections, sorted by (end_frame, keyword index)."""
        return [self.detection(*h) for h in sorted(hits, key=lambda h: (h[2], h[0]))]

    def bests(self, scores, spans):
        """[N][K] Best tuples from ops.kws_best's host tensors"""
        sc, sp = scores.tolist(), spans.tolist()
        return [[Best(self.keywords[k], k, sp[n][k][0], sp[n][k][1], sc[n][k], sc[n][k] / len(self.label_ids[k]))
                 for k in range(len(self.keywords))] for n in range(len(sc))]

    def stream(self, num_streams, device="cuda"):
        """A KeywordStream of num_streams streams on `device`."""
        return KeywordStream(self, num_streams, device)

    def spot(self, out, sizes, kind="probs", return_best=False):
        """out: (N, T', C) device tensor as DeepSpeech.forward returns it -- probabilities in eval mode (kind="probs"), logits
        in training mode ("logits"), or "log_probs"; the transposed view is read in place.  sizes: [N] valid frames.  Returns per
        clip the list of Detections sorted by (end_frame, keyword index); with return_best also the [N][K] Best tuples.  The hits
        beyond max_hits per keyword and clip are counted in ``last_dropped`` (per clip) and warned about."""
        if kind not in KINDS:
            raise ValueError("kind must be one of %s, got %r" % (sorted(KINDS), kind))
        if out.dtype != torch.float32:
            out = out.float()
        ks = KeywordStream(self, out.shape[0], out.device)
        dets = ks.feed(out, sizes, kind=kind, end=True)
        self.last_dropped = list(ks.dropped)
        if any(self.last_dropped):
            warnings.warn("keyword spotting dropped %d hits beyond max_hits=%d per keyword" % (sum(self.last_dropped), self.max_hits))
        return (dets, ks.best()) if return_best else dets


class KeywordStream:
    """The spotter's device state for N streams (ops.kws_open).  ``feed`` returns the detections that the feed emits, with
    absolute frames; over any chunking they are ``spot``'s on the concatenated frames."""

    def __init__(self, spotter, num_streams, device="cuda"):
        from . import ops
        self._ops, self.spotter, self.num_streams = ops, spotter, int(num_streams)
        self.h = ops.kws_open(self.num_streams, spotter.lanes, len(spotter.keywords), spotter.hold, spotter.max_hits,
                              spotter.blank_index, device)
        self.dropped = [0] * self.num_streams          # per stream: the hits beyond max_hits per keyword of a feed, summed

    def _emit(self, hits, dropped):
        for n, d in enumerate(dropped):
            self.dropped[n] += d
        return [self.spotter.detections(h) for h in hits]

    def feed(self, probs, sizes=None, kind="probs", end=None):
        """probs: (N, Tc, C) device chunk (what `kind` says); sizes: [N] ints (None = Tc), 0 leaves a stream as it is.  end: None,
        True or the streams whose utterance ends with this chunk (their open candidate is emitted).  Returns per stream the
        Detections emitted by this feed: a hit comes back in the feed in which its hold runs out, or at the end."""
        if kind not in KINDS:
            raise ValueError("kind must be one of %s, got %r" % (sorted(KINDS), kind))
        if probs.dtype != torch.float32:
            probs = probs.float()
        return self._emit(*self._ops.kws_feed(self.h, probs, sizes, KINDS[kind], end))

    def end(self, streams=None):
        """The open candidates of `streams` (None = all) are emitted; returns them per stream.  The lattice runs on."""
        return self._emit(*self._ops.kws_feed(self.h, None, None, 1, True if streams is None else list(streams)))

    def reset(self, streams=None):
        """Streams `streams` (None = all) start again at frame 0 with no path, candidate or best; the others are untouched."""
        self._ops.kws_reset(self.h, streams)
        for n in (range(self.num_streams) if streams is None else streams):
            self.dropped[int(n)] = 0

    def best(self):
        """[N][K] Best tuples: the largest end score of every (stream, keyword) so far, whatever the threshold."""
        return self.spotter.bests(*self._ops.kws_best(self.h))

    @property
    def frames(self):
        """frames consumed per stream (host ints; waits for the device)"""
        return self._ops.kws_frames(self.h)
