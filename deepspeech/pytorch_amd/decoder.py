"""Greedy decoder + WER / CER with the reference's interfaces (``deepspeech_pytorch.decoder.GreedyDecoder``,
decoder.py:117-181; ``deepspeech_pytorch.validation.WordErrorRate / CharErrorRate``, validation.py:13-132), so that
``DeepSpeech.validation_step`` (model.py:251-271) works exactly as in the reference.

The arg-max + repeat collapse + blank removal of ``decode`` runs on the device (ds2_greedy_decode); only the surviving
labels travel to the host.  String building and the edit distance are host-side bookkeeping, as in the reference.
``BeamCTCDecoder`` (decoder.py:56-117) runs CTC prefix beam search on the device (ds2_beam_decode), with a word n-gram language
model from an ARPA file when ``lm_path`` is given (ds2_beam_decode_lm, lm.py).
When the reference's metric classes are importable the model uses THEM (with this decoder inside); the classes below are the
stand-ins for images without torchmetrics / Levenshtein."""
import collections

import torch

from . import ops


class GreedyDecoder:
    def __init__(self, labels, blank_index=0):
        self.labels = labels
        self.int_to_char = dict((i, c) for (i, c) in enumerate(labels))
        self.blank_index = blank_index
        space_index = len(labels)          # decoder.py:36-38: out of range unless ' ' is a label
        if ' ' in labels:
            space_index = labels.index(' ')
        self.space_index = space_index

    # ---- reference decoder.py:121-162 (host-side string building; used for the TARGET side by the metrics) ----------
    def convert_to_strings(self, sequences, sizes=None, remove_repetitions=False, return_offsets=False):
        strings, offsets = [], ([] if return_offsets else None)
        for x in range(len(sequences)):
            seq_len = sizes[x] if sizes is not None else len(sequences[x])
            string, string_offsets = self.process_string(sequences[x], seq_len, remove_repetitions)
            strings.append([string])
            if return_offsets:
                offsets.append([string_offsets])
        return (strings, offsets) if return_offsets else strings

    def process_string(self, sequence, size, remove_repetitions=False):
        seq = [int(v) for v in (sequence.tolist() if hasattr(sequence, "tolist") else sequence)][:int(size)]
        chars, offsets = [], []
        for i, v in enumerate(seq):
            if v != self.blank_index:
                if remove_repetitions and i != 0 and v == seq[i - 1]:
                    continue
                chars.append(' ' if v == self.space_index else self.int_to_char[v])
                offsets.append(i)
        return ''.join(chars), torch.tensor(offsets, dtype=torch.int)

    # ---- reference decoder.py:164-181, on the device -------------------------------------------------------------------
    def decode(self, probs, sizes=None):
        """probs: (N, T', C) scores on a HIP device.  Returns (strings, offsets) exactly as the reference: strings[n] = [str],
        offsets[n] = [int tensor of the frame of every emitted character]."""
        toks, offs = ops.greedy_decode(probs, sizes, self.blank_index)
        strings = [[''.join(' ' if v == self.space_index else self.int_to_char[v] for v in t)] for t in toks]
        return strings, [[o.to(torch.int)] for o in offs]

    def decode_words(self, probs, sizes=None, confidence=None, frame_seconds=None, kind="probs"):
        """decode with word and character timings and confidences: [Hypothesis] per clip (confidence.py; score and acoustic are
        None).  A character's span is the arg-max run it was collapsed from.  kind: what probs holds, as ForcedAligner.align's;
        confidence: a Confidence (None = Confidence()); frame_seconds: the duration of a frame, for start_s / end_s."""
        from . import align, confidence as _conf
        conf = _conf.Confidence() if confidence is None else confidence
        if not isinstance(conf, _conf.Confidence):
            raise ValueError("confidence must be a Confidence, got %r" % (confidence,))
        if kind not in align.KINDS:
            raise ValueError("kind must be one of %s, got %r" % (sorted(align.KINDS), kind))
        conf.check_classes(probs.shape[2])
        if probs.shape[0] == 0 or probs.shape[1] == 0:
            return [_conf.Hypothesis('', None, None, None, [], [], []) for _ in range(probs.shape[0])]
        if not probs.is_cuda:
            probs = probs.to("cuda")
        words = dict(space=self.space_index, measure=conf.measure, alpha=conf.alpha, aggregate=conf.aggregate,
                     word_aggregate=conf.word_aggregate, nbest=1, kind=kind)
        labels, _, res = ops.greedy_decode(probs, sizes, self.blank_index, _words=words)
        return [_conf.make_hypothesis(labels[n][0], self.int_to_char, self.space_index, res[n][0], None, None, frame_seconds)
                for n in range(len(labels))]

    def stream(self, num_streams, device="cuda", endpoint=None, confidence=None, max_frames=None):
        """A GreedyStream: decode for num_streams streams that arrive chunk by chunk.  endpoint: an Endpointer cuts every stream
        into segments (EndpointedGreedyStream).  confidence: a Confidence makes the stream keep its frames on the device, up to
        max_frames per stream (required then; 4 * len(labels) bytes per frame and stream), and gives it ``words()``; with an
        endpoint the frames live in a ring of ring_capacity(endpoint) frames instead, max_frames plays no part, the finished
        segments carry ``.hypotheses`` and ``best_words()`` gives the open segment's partial."""
        if endpoint is not None:
            return EndpointedGreedyStream(self, num_streams, device, endpoint, confidence)
        return GreedyStream(self, num_streams, device, confidence, max_frames)


class Endpointer:
    """The rule that cuts an endless stream of CTC posteriors into utterances.  Frame t is silent iff
    its blank probability > blank_threshold (fp32, strict).  A segment ends at the first frame where, in this order, "silence":
    it has a non-silent frame and min_trailing silent ones at its end; "leading": it has max_leading silent frames and no other;
    "length": it has max_segment frames.  The counts are output frames (20 ms): the defaults are 1 s, 5 s and 20 s, the
    conventional values for CTC endpointing, not tuned on any data."""

    def __init__(self, blank_threshold=0.8, min_trailing=50, max_leading=250, max_segment=1000):
        self.blank_threshold, self.min_trailing, self.max_leading, self.max_segment = ops.endpoint_rule_checks(
            blank_threshold, min_trailing, max_leading, max_segment)

    @property
    def sub_feed(self):
        """the longest chunk that cannot hold two endpoints of one stream: two endpoints lie at least min(min_trailing + 1,
        max_leading, max_segment) frames apart"""
        return min(self.min_trailing, self.max_leading, self.max_segment)

    def check_max_frames(self, max_frames):
        if self.max_segment > int(max_frames):
            raise ValueError("max_segment=%d passes the stream's max_frames=%d: a segment must fit the node pool"
                             % (self.max_segment, int(max_frames)))

    def __repr__(self):
        return "Endpointer(blank_threshold=%r, min_trailing=%d, max_leading=%d, max_segment=%d)" % (
            self.blank_threshold, self.min_trailing, self.max_leading, self.max_segment)


# a finished utterance: its number in the stream, its first and last frame (absolute; end = start - 1 for an empty "final" one),
# why it ended, and its best beams as decode_beams gives them on probs[start : end + 1], the offsets as absolute stream frames;
# acoustic: the beams' acoustic -log p; labels: the beams as label indices
Segment = collections.namedtuple("Segment", "index start end reason strings offsets scores acoustic labels",
                                 defaults=(None, None))


class WordSegment(Segment):
    """A Segment of a stream opened with confidence=: the same fields, equal to the plain tuple, and two attributes:
    ``hypotheses``, the confidence.Hypothesis of every kept beam (word and character frames are absolute stream frames, like the
    offsets), and ``confidence``, the top beam's (None without words)."""

    def __new__(cls, segment, hypotheses):
        self = super().__new__(cls, *segment)
        self.hypotheses = hypotheses
        self.confidence = hypotheses[0].confidence if hypotheses else None
        return self


RING_SLOTS = 8      # finished segments the device keeps per endpointed beam stream; a fetch happens at least every RING_SLOTS device feeds


def ring_capacity(endpoint, slots=RING_SLOTS):
    """Frames an endpointed stream keeps for the confidence pass.  At a fetch the frames still needed run from the start of the
    oldest segment not yet fetched (or of the open one) to the newest frame.  A segment has at most max_segment frames; one that
    is not yet fetched ended after the last fetch, and since then at most `slots` device feeds of at most sub_feed frames each
    were consumed: max_segment + slots * sub_feed (tests/test_confidence_host.py simulates feed and fetch schedules against it)."""
    return endpoint.max_segment + int(slots) * endpoint.sub_feed


def split_feed(sizes, limit):
    """Cuts one feed into sub-feeds of at most `limit` frames per stream: [(t0, t1, sub_sizes)], sub-feed k holding the chunk's
    frames [t0, t1) = [k * limit, ...) and stream n taking its first sub_sizes[n] of them.  Sub-feeds that no stream takes part in
    are left out; per stream the sub-feeds' frames concatenate to its sizes[n] frames."""
    limit = int(limit)
    if limit < 1:
        raise ValueError("the sub-feed limit must be >= 1, got %d" % limit)
    out = []
    for t0 in range(0, max(sizes, default=0), limit):
        sub = [min(max(v - t0, 0), limit) for v in sizes]
        out.append((t0, t0 + max(sub), sub))
    return out


def _stream_sizes(sizes, N, Tc):
    """the host ints of a feed's sizes (None = the whole chunk for every stream)"""
    if sizes is None:
        return [Tc] * N
    sz = [int(v) for v in (sizes.tolist() if hasattr(sizes, "tolist") else sizes)]
    if len(sz) != N or any(not 0 <= v <= Tc for v in sz):
        raise ValueError("sizes must be %d ints in [0, %d] (the chunk's frames), got %s" % (N, Tc, sz))
    return sz


def _conf_settings(decoder, confidence, nbest=1, kind="probs"):
    """(Confidence, the settings dict of ops' confidence pass) for a stream opened with confidence= (None: (None, None))"""
    if confidence is None:
        return None, None
    from . import confidence as _conf
    if not isinstance(confidence, _conf.Confidence):
        raise ValueError("confidence must be a Confidence, got %r" % (confidence,))
    confidence.check_classes(len(decoder.labels))
    return confidence, dict(space=decoder.space_index, measure=confidence.measure, alpha=confidence.alpha,
                            aggregate=confidence.aggregate, word_aggregate=confidence.word_aggregate, nbest=int(nbest), kind=kind)


def _hypotheses(decoder, labels, res, scores=None, acoustic=None, frame_seconds=None, shifts=None):
    """[[Hypothesis] per rank] per stream from ops._words_to_host's values; shifts[n]: added to stream n's frames"""
    from . import confidence as _conf
    with _conf.building_tuples():
        return [[_conf.make_hypothesis(labels[n][r], decoder.int_to_char, decoder.space_index, res[n][r],
                                       None if scores is None else float(scores[n, r]),
                                       None if acoustic is None else float(acoustic[n, r]), frame_seconds,
                                       0 if shifts is None else int(shifts[n]))
                 for r in range(len(labels[n]))] for n in range(len(labels))]


class GreedyStream:
    """GreedyDecoder.decode on streams that arrive in chunks (ds2_greedy_stream_feed): the previous frame's arg-max and the frame
    count of every stream stay on the device, so a repeated label or a run of blanks across a chunk boundary is collapsed as in the
    whole utterance.  ``text[n]`` is the transcript so far, ``offsets[n]`` its frames, ``frames[n]`` the frames consumed."""

    def __init__(self, decoder, num_streams, device="cuda", confidence=None, max_frames=None):
        self.decoder, self.num_streams = decoder, int(num_streams)
        self._carry = torch.zeros((self.num_streams, 2), dtype=torch.int32, device=device)
        self.confidence, self._wc = _conf_settings(decoder, confidence)
        self._store, self._toks, self.max_frames = None, None, None
        if confidence is not None:
            if max_frames is None:
                raise ValueError("a greedy stream with confidence= keeps its frames: it needs max_frames")
            self.max_frames = int(max_frames)
            self._store = ops.frame_store_open(self.num_streams, self.max_frames, len(decoder.labels), self._carry.device)
        self.reset()

    def words(self, frame_seconds=None):
        """Per stream the Hypothesis (confidence.py) of the whole stream so far: GreedyDecoder.decode_words on the frames consumed.
        The transcript so far is uploaded in one copy."""
        if self._store is None:
            raise ValueError("words() needs a stream opened with confidence=")
        hyps = [[(self._toks[n], self.offsets[n].tolist())] for n in range(self.num_streams)]
        labels, _, res = ops.host_hypotheses_words(self._store.rows, self._store.count, hyps, self.decoder.blank_index, self._wc,
                                                   self._wc["kind"])
        return [h[0] for h in _hypotheses(self.decoder, labels, res, frame_seconds=frame_seconds)]

    def reset(self, streams=None):
        """Streams `streams` (None = all) start again."""
        if self._store is not None:
            ops.frame_store_reset(self._store, streams)
            if streams is None:
                self._toks = [[] for _ in range(self.num_streams)]
            else:
                for n in streams:
                    self._toks[n] = []
        if streams is None:
            self._carry.zero_()
            self.text = [''] * self.num_streams
            self.offsets = [torch.zeros(0, dtype=torch.int) for _ in range(self.num_streams)]
            self.frames = [0] * self.num_streams
        else:
            for n in streams:
                self._carry[n].zero_()
                self.text[n], self.offsets[n], self.frames[n] = '', torch.zeros(0, dtype=torch.int), 0

    def feed(self, probs, sizes=None):
        """probs: (N, Tc, C) scores of the next chunk (device or host tensor); sizes: host ints per stream (None = Tc), 0 leaving a
        stream as it is.  Returns (strings, offsets) of what the chunk adds: strings[n] a str, offsets[n] an int tensor of frames
        counted from the start of the stream."""
        d = self.decoder
        if not probs.is_cuda:
            probs = probs.to(self._carry.device)
        sz = _stream_sizes(sizes, self.num_streams, probs.shape[1])
        if self._store is not None:
            for n, v in enumerate(sz):
                if self.frames[n] + v > self.max_frames:
                    raise ValueError("stream %d: %d frames consumed + %d fed pass max_frames=%d"
                                     % (n, self.frames[n], v, self.max_frames))
            if probs.shape[1]:
                x = probs if probs.dtype == torch.float32 else probs.float()
                ops.frame_store_append(self._store, x if x.stride(2) == 1 else x.contiguous(),
                                       None if sizes is None else ops._sizes_to_device(sz, x.device))
        toks, offs = ops.greedy_stream_feed(probs, None if sizes is None else torch.tensor(sz, dtype=torch.int32), d.blank_index,
                                            self._carry)
        if self._store is not None:
            for n in range(self.num_streams):
                self._toks[n] = self._toks[n] + toks[n]
        strings = [''.join(' ' if v == d.space_index else d.int_to_char[v] for v in t) for t in toks]
        offs = [o.to(torch.int) for o in offs]
        for n in range(self.num_streams):
            self.text[n] += strings[n]
            self.offsets[n] = torch.cat([self.offsets[n], offs[n]])
            self.frames[n] += sz[n]
        return strings, offs


class EndpointedGreedyStream(GreedyStream):
    """A GreedyStream that an Endpointer cuts into segments on the device (ds2_endpoint_feed in front of every greedy feed).
    ``text[n]`` / ``offsets[n]`` are the partial of the OPEN segment, ``segments()`` drains the finished ones; every segment's
    text and offsets are GreedyDecoder.decode's on its frames alone, the offsets counted from the start of the stream.
    ``frames[n]`` counts all the frames consumed.  The events ride on the fetch that every greedy feed makes anyway."""

    def __init__(self, decoder, num_streams, device, endpoint, confidence=None):
        e = self.endpoint = endpoint
        self._ep = ops.endpoint_open(num_streams, decoder.blank_index, e.blank_threshold, e.min_trailing, e.max_leading,
                                     e.max_segment, device)
        self._start, self._labels = [0] * int(num_streams), [[] for _ in range(int(num_streams))]
        self._done = [[] for _ in range(int(num_streams))]
        super().__init__(decoder, num_streams, self._ep.device)
        self.confidence, self._wc = _conf_settings(decoder, confidence)
        self._fresh = []                   # (stream, position in _done) of the segments that still wait for their hypotheses
        if confidence is not None:
            self._toks = [[] for _ in range(self.num_streams)]
            self._store = ops.frame_store_open(self.num_streams, ring_capacity(e), len(decoder.labels), self._ep.device)

    def _attach(self):
        """the hypotheses of the segments finished in the last device feed (at most one per stream): one upload, one pass"""
        if self._store is None or not self._fresh:
            self._fresh = []
            return
        N = self.num_streams
        sizes, starts, hyps = [0] * N, [0] * N, [[([], [])] for _ in range(N)]
        for n, i in self._fresh:
            s = self._done[n][i]
            sizes[n], starts[n] = s.end - s.start + 1, s.start
            hyps[n] = [(s.labels[0], (s.offsets[0] - s.start).tolist())]
        labels, _, res = ops.ring_segments_words(self._store, [(sizes, starts, hyps)], self.decoder.blank_index, self._wc)[0]
        hy = _hypotheses(self.decoder, labels, res, shifts=starts)
        for n, i in self._fresh:
            self._done[n][i] = WordSegment(self._done[n][i], hy[n])
        self._fresh = []

    def words(self, frame_seconds=None):
        """Per stream the Hypothesis of the OPEN segment's partial (frames absolute); finished segments carry theirs."""
        if self._store is None:
            raise ValueError("words() needs a stream opened with confidence=")
        st = ops.endpoint_state(self._ep).tolist()
        starts = [r[0] for r in st]
        hyps = [[(self._labels[n], (self.offsets[n] - starts[n]).tolist())] for n in range(self.num_streams)]
        labels, _, res = ops.ring_segments_words(self._store, [([r[3] - r[0] for r in st], starts, hyps)],
                                                 self.decoder.blank_index, self._wc)[0]
        return [h[0] for h in _hypotheses(self.decoder, labels, res, frame_seconds=frame_seconds, shifts=starts)]

    best_words = words

    def reset(self, streams=None):
        """Streams `streams` (None = all) start again at frame 0 and segment 0; their undrained segments are dropped."""
        super().reset(streams)
        ops.endpoint_reset(self._ep, streams)
        for n in (range(self.num_streams) if streams is None else streams):
            self._start[n], self._labels[n], self._done[n] = 0, [], []

    def _finish(self, n, reason, start, end, index):
        self._done[n].append(Segment(index, start, end, reason, [self.text[n]], [self.offsets[n]], None, None, [self._labels[n]]))
        self._fresh.append((n, len(self._done[n]) - 1))
        self._carry[n].zero_()
        self.text[n], self.offsets[n], self._labels[n], self._start[n] = '', torch.zeros(0, dtype=torch.int), [], end + 1

    def feed(self, probs, sizes=None):
        """GreedyStream.feed; a chunk longer than endpoint.sub_feed frames is fed in pieces.  Returns (strings, offsets) of what
        the chunk adds per stream, over all the segments it touches."""
        d = self.decoder
        if not probs.is_cuda:
            probs = probs.to(self._carry.device)
        if probs.dtype != torch.float32:
            probs = probs.float()
        if probs.stride(2) != 1:
            probs = probs.contiguous()
        sz = _stream_sizes(sizes, self.num_streams, probs.shape[1])
        added = [''] * self.num_streams
        added_offs = [[] for _ in range(self.num_streams)]
        for t0, t1, take in split_feed(sz, self.endpoint.sub_feed):
            x = probs[:, t0:t1]
            while any(take):
                cut, rest, ev = ops.endpoint_feed(self._ep, x, torch.tensor(take, dtype=torch.int32))
                if self._store is not None:
                    ops.frame_store_append(self._store, x, cut)
                toks, offs = ops.greedy_stream_feed(x, cut, d.blank_index, self._carry)
                take, reason, start, end, index = torch.cat([rest[None], ev]).cpu().tolist()
                for n in range(self.num_streams):
                    s = ''.join(' ' if v == d.space_index else d.int_to_char[v] for v in toks[n])
                    o = offs[n].to(torch.int) + self._start[n]
                    self.text[n] += s
                    self.offsets[n] = torch.cat([self.offsets[n], o])
                    self._labels[n] = self._labels[n] + toks[n]
                    added[n] += s
                    added_offs[n].append(o)
                    if reason[n]:
                        self._finish(n, ops.ENDPOINT_REASONS[reason[n]], start[n], end[n], index[n])
                self._attach()
                if any(take):
                    x = ops.endpoint_gather(x, cut, rest)         # the frames after the cut: the next segment's first
        self.frames = [f + v for f, v in zip(self.frames, sz)]
        return added, [torch.cat(o) if o else torch.zeros(0, dtype=torch.int) for o in added_offs]

    def end(self, streams=None):
        """The open segment of streams `streams` (None = all) ends with reason "final"; it may be empty."""
        streams = list(range(self.num_streams)) if streams is None else [int(n) for n in streams]
        reason, start, end, index = ops.endpoint_close(self._ep, streams).cpu().tolist()
        for n in streams:
            self._finish(n, ops.ENDPOINT_REASONS[reason[n]], start[n], end[n], index[n])
        self._attach()

    def segments(self):
        """Per stream the list of Segments finished since the last call."""
        out, self._done = self._done, [[] for _ in range(self.num_streams)]
        return out


class BeamCTCDecoder:
    """CTC prefix beam search with the reference's interface (``deepspeech_pytorch.decoder.BeamCTCDecoder``, decoder.py:56-117),
    run on the device (ds2_beam_decode) instead of the ctcdecode library on a host copy.  ``lm_path`` names an ARPA text file of
    a word n-gram model of order 1 to 5 (KenLM binaries do not load); every completed word then adds
    ``alpha * ln P(word | context) + beta`` to its beam, and with ``lexicon=True`` (ctcdecode's dictionary, the default) only
    beams that spell vocabulary words survive.  ``alpha`` / ``beta`` are ignored without an LM (as in ctcdecode) and
    ``num_processes`` is ignored (no CPU threads).  ``lexicon`` is a keyword of this class only.

    ``hotwords`` is a list of phrases the search should prefer (hotwords.py; DESIGN.md "ds2_beam", hot words): strings, or
    (string, weight) pairs, the weight in natural-log units per non-space label (default ``hotword_weight``).  With an LM a hot
    word outside its vocabulary is charged ``ln P = hot_oov_logp`` in place of -1000 and survives the lexicon.  ``None`` or an empty
    list runs the entry points without hot words.  These three are keywords of this class only.

    ``lm_unit`` says what the n-gram model's units are: ``"word"`` (the default), ``"char"`` -- every label is an event of the
    model, ``alpha * ln P(label | the last order - 1 labels) + beta``, for label sets without word boundaries (DESIGN.md
    "ds2_beam", character language model) -- or ``"auto"``, which picks ``"char"`` exactly when every unigram of the file other
    than ``<s>``, ``</s>``, ``<unk>`` is one code point long (ctcdecode's test).  ``self.lm_unit`` holds the resolved value.  In
    character mode a label is looked up in the file as it is written in ``labels``; the space label as ``space_token`` (e.g.
    ``"|"``) when that is given and otherwise not at all (it is out of vocabulary).  No space label is needed, ``lexicon`` is
    ignored, there is no end-of-utterance term, and hot words are refused (ValueError).  Keywords of this class only."""

    def __init__(self, labels, lm_path=None, alpha=0, beta=0, cutoff_top_n=40, cutoff_prob=1.0, beam_width=100,
                 num_processes=4, blank_index=0, lexicon=True, hotwords=None, hotword_weight=2.0, hot_oov_logp=-11.5,
                 lm_unit="word", space_token=None):
        self.lm, self.lexicon, self._tables = None, bool(lexicon), {}
        if lm_unit not in ("word", "char", "auto"):
            raise ValueError("lm_unit must be 'word', 'char' or 'auto', got %r" % (lm_unit,))
        self.lm_unit, self.space_token = "word", space_token
        if lm_path:
            from . import lm as _lm
            lm = _lm.load_arpa(lm_path)          # ValueError unless it is an ARPA text file of order 1 to 5
            if lm_unit == "auto":
                lm_unit = "char" if _lm.is_character_based(lm) else "word"
            if lm_unit == "word" and (' ' not in labels or labels.index(' ') == blank_index):
                raise ValueError("BeamCTCDecoder: a language model needs a space label other than the blank to end words")
            if lm_unit == "char":
                _lm.char_ids(lm, labels, blank_index, space_token)       # ValueError for a space_token that is no unigram
            self.lm, self.lm_unit = lm, lm_unit
        self.labels = labels
        self.int_to_char = dict((i, c) for (i, c) in enumerate(labels))
        self.blank_index = blank_index
        space_index = len(labels)          # decoder.py:36-38
        if ' ' in labels:
            space_index = labels.index(' ')
        self.space_index = space_index
        self.lm_path, self.alpha, self.beta = lm_path, alpha, beta
        self.cutoff_top_n, self.cutoff_prob, self.beam_width = int(cutoff_top_n), float(cutoff_prob), int(beam_width)
        self.num_processes = num_processes
        self.hotword_weight, self.hot_oov_logp = float(hotword_weight), float(hot_oov_logp)
        if self.hot_oov_logp != self.hot_oov_logp or abs(self.hot_oov_logp) > 3.4e38:
            raise ValueError("hot_oov_logp must be a finite fp32 value, got %r" % (hot_oov_logp,))
        self.set_hotwords(hotwords)

    def set_hotwords(self, hotwords):
        """Replaces the hot phrases (None or an empty list: none).  ValueError, naming the phrase, for one that breaks the rules of
        hotwords.py.  Calls and streams opened from now on use the new table; an open BeamStream keeps the one it was opened with."""
        hotwords = list(hotwords) if hotwords else []
        table = None
        if hotwords and self.lm is not None and self.lm_unit == "char":
            raise ValueError("BeamCTCDecoder: hot words are defined on word boundaries and are not supported with a character "
                             "language model (lm_unit='char')")
        if hotwords:
            from . import hotwords as _hot
            table = _hot.build_table(hotwords, self.labels, self.blank_index, self.hotword_weight)
        self.hotwords, self._hot_host, self._hot_dev = hotwords, table, {}

    def _hot_table(self, device):
        """The hot-word table on `device` (None without hot words): uploaded on first use, then kept until set_hotwords."""
        if self._hot_host is None:
            return None
        if device not in self._hot_dev:
            self._hot_dev[device] = torch.from_numpy(self._hot_host).to(device)
        return self._hot_dev[device]

    def _hot_args(self, device):
        """The hot dict of ops.beam_search / ops.beam_stream_open for `device`, None without hot words."""
        ht = self._hot_table(device)
        return None if ht is None else dict(space=self.space_index, table=ht, oov_logp=self.hot_oov_logp)

    def decode_beams(self, probs, sizes=None):
        """(strings, offsets, scores): strings[n] = beam_width transcripts (best first), offsets[n] = the matching int tensors of
        frames, scores = host (N, beam_width) float tensor of -log p, with an LM -(log p + lm) (lower is better; +inf where no
        beam is alive).  The reference's run_transcribe passes out.cpu() (inference.py:96-98): a host tensor is moved over."""
        return self.decode_beams_detailed(probs, sizes)[:3]

    def _lm_tables(self, device):
        """The LM's two tables on `device`: built and uploaded on first use, then kept."""
        if device not in self._tables:
            from . import lm as _lm
            if self.lm_unit == "char":           # (label ids, n-gram table)
                wt, gt = _lm.build_char_tables(self.lm, self.labels, self.blank_index, self.space_token)
            else:
                wt, gt = _lm.build_tables(self.lm, self.labels, self.blank_index, self.space_index)
            self._tables[device] = (torch.from_numpy(wt).to(device), torch.from_numpy(gt).to(device))
        return self._tables[device]

    def _lm_args(self, device):
        """The lm dict of ops.beam_search / ops.beam_stream_open for `device`, None without a language model."""
        if self.lm is None:
            return None
        wt, gt = self._lm_tables(device)
        if self.lm_unit == "char":
            return dict(unit="char", label_ids=wt, ngram_table=gt, order=self.lm.order, bos=self.lm.bos, alpha=self.alpha,
                        beta=self.beta)
        return dict(space=self.space_index, word_table=wt, ngram_table=gt, order=self.lm.order, bos=self.lm.bos, alpha=self.alpha,
                    beta=self.beta, lexicon=self.lexicon)

    def _search(self, probs, sizes, words=None):
        """The one-shot search in the form this decoder is set up for (plain, hot words, LM, LM with hot words); words: the
        settings of ops' confidence pass for decode_words, None for the plain results."""
        lm, hot = self._lm_args(probs.device), self._hot_args(probs.device)
        if lm is None and hot is not None:      # by its own name: test_gpu_beam_hot counts the calls of ops.beam_decode_hot
            return ops.beam_decode_hot(probs, sizes, self.blank_index, self.beam_width, self.cutoff_top_n, self.cutoff_prob,
                                       hot["space"], hot["table"], _words=words)
        return ops.beam_search(probs, sizes, self.blank_index, self.beam_width, self.cutoff_top_n, self.cutoff_prob, lm, hot,
                               _words=words)

    def nbest_device(self, probs, sizes, nbest):
        """The label rows of the best `nbest` beams of every clip, left on the device for the training step (mwer.MWERLoss):
        tokens [nbest][N][T'] int32 and lens [nbest][N] int32, rank-major (row r * N + n, ds2_error_counts' convention), lens = -1
        where the search's score is +inf (fewer beams alive than asked for); entries past a row's length are not initialised.  The search runs in the form this decoder is set up
        for (plain, LM, character LM, hot words); only the label rows are used, so scores and frames stay behind.  Nothing
        travels to the host."""
        if not 1 <= int(nbest) <= self.beam_width:
            raise ValueError("nbest must be in [1, beam_width=%d], got %r" % (self.beam_width, nbest))
        if not (torch.is_tensor(probs) and probs.is_cuda):
            raise ValueError("nbest_device needs a HIP device tensor; there is no CPU fallback")
        from .mwer import rank_major
        K = int(nbest)
        buf, lens, scores = ops.beam_search_device(probs, sizes, self.blank_index, self.beam_width, self.cutoff_top_n, self.cutoff_prob,
                                                   self._lm_args(probs.device), self._hot_args(probs.device))
        return rank_major(buf[0], lens, scores[0], K)

    def decode_beams_detailed(self, probs, sizes=None):
        """(strings, offsets, scores, acoustic): decode_beams' three values and the acoustic -log p of the same beams.  With an
        LM, scores = acoustic - lm (the total that ranked the beams); without one the two are equal."""
        if not probs.is_cuda:
            probs = probs.to("cuda")
        toks, offs, scores, acoustic = self._search(probs, sizes)
        strings = [[''.join(self.int_to_char[v] for v in t) for t in beams] for beams in toks]
        offsets = [[o.to(torch.int) for o in beams] for beams in offs]
        return strings, offsets, scores, acoustic

    def decode_words(self, probs, sizes=None, confidence=None, nbest=1, frame_seconds=None):
        """The best `nbest` beams of every clip with word and character timings and confidences: [[Hypothesis] * nbest] per clip
        (confidence.py).  text, score and acoustic are decode_beams_detailed's of the same rank; the spans and confidences come
        from one device pass over the search's own buffers (ds2_confidence), so only the top nbest ranks travel to the host.
        confidence: a Confidence (None = Confidence()); frame_seconds: the duration of a frame, for start_s / end_s."""
        from . import confidence as _conf
        conf = _conf.Confidence() if confidence is None else confidence
        if not isinstance(conf, _conf.Confidence):
            raise ValueError("confidence must be a Confidence, got %r" % (confidence,))
        if not 1 <= int(nbest) <= self.beam_width:
            raise ValueError("nbest must be in [1, beam_width=%d], got %r" % (self.beam_width, nbest))
        conf.check_classes(probs.shape[2])
        if not probs.is_cuda:
            probs = probs.to("cuda")
        if probs.shape[0] == 0 or probs.shape[1] == 0:       # no frames: the empty string alone
            _, _, scores, acoustic = self.decode_beams_detailed(probs, sizes)
            return [[_conf.Hypothesis('', float(scores[n, r]), float(acoustic[n, r]), None, [], [], [])
                     for r in range(int(nbest))] for n in range(probs.shape[0])]
        if probs.dtype != torch.float32:
            probs = probs.float()
        words = dict(space=self.space_index, measure=conf.measure, alpha=conf.alpha, aggregate=conf.aggregate,
                     word_aggregate=conf.word_aggregate, nbest=int(nbest))
        labels, _, res, scores, acoustic = self._search(probs, sizes, words)
        with _conf.building_tuples():
            return [[_conf.make_hypothesis(labels[n][r], self.int_to_char, self.space_index, res[n][r], float(scores[n, r]),
                                           float(acoustic[n, r]), frame_seconds)
                     for r in range(len(labels[n]))] for n in range(len(labels))]

    def decode_grid_device(self, probs, sizes, points, max_ws_bytes=1 << 30):
        """The top beam at every (alpha, beta) of `points`, left on the device: ops.beam_decode_lm_grid's five tensors
        (tokens [G, N, T'], offsets, lens [G, N], scores, acoustic).  ``self.alpha`` / ``self.beta`` play no part."""
        if self.lm is None:
            raise ValueError("BeamCTCDecoder.decode_grid searches language-model weights: it needs lm_path")
        if self.hotwords:
            raise ValueError("BeamCTCDecoder.decode_grid does not support hot words: the weight search is not boosted; call "
                             "set_hotwords(None) first")
        points = [(float(a), float(b)) for a, b in points]
        if not points:
            raise ValueError("decode_grid needs at least one (alpha, beta) point")
        if not probs.is_cuda:
            probs = probs.to("cuda")
        lm = self._lm_args(probs.device)
        if self.lm_unit == "char":
            return ops.beam_decode_clm_grid(probs, sizes, self.blank_index, self.beam_width, self.cutoff_top_n, self.cutoff_prob,
                                            lm["label_ids"], lm["ngram_table"], lm["order"], lm["bos"],
                                            [a for a, _ in points], [b for _, b in points], max_ws_bytes)
        return ops.beam_decode_lm_grid(probs, sizes, self.blank_index, self.beam_width, self.cutoff_top_n, self.cutoff_prob,
                                       lm["space"], lm["word_table"], lm["ngram_table"], lm["order"], lm["bos"],
                                       [a for a, _ in points], [b for _, b in points], lm["lexicon"], max_ws_bytes)

    def decode_grid(self, probs, sizes, points):
        """decode's best transcript at every (alpha, beta) of `points`, from one launch: strings[g][n], offsets[g][n] (int tensor
        of frames) and a host (G, N) float tensor of scores, equal to decode_beams' rank 0 with alpha, beta = points[g]."""
        toks, offs, lens, scores, _ = self.decode_grid_device(probs, sizes, points)
        ln = lens.cpu().numpy()
        G, N = ln.shape
        width = max(int(ln.max()), 1) if ln.size else 1
        th, oh = toks[:, :, :width].cpu().numpy(), offs[:, :, :width].cpu()
        strings = [[''.join(self.int_to_char[v] for v in th[g, n, :ln[g, n]].tolist()) for n in range(N)] for g in range(G)]
        offsets = [[oh[g, n, :ln[g, n]].to(torch.int) for n in range(N)] for g in range(G)]
        return strings, offsets, scores.cpu()

    def decode(self, probs, sizes=None):
        """probs: (N, T', C) probabilities (device or host tensor).  Returns (strings, offsets) in the reference's shapes:
        strings[n] is a list of beam_width transcripts, offsets[n] the matching list of int tensors."""
        strings, offsets, _ = self.decode_beams(probs, sizes)
        return strings, offsets

    def stream(self, num_streams, max_frames, device="cuda", endpoint=None, nbest=1, confidence=None):
        """A BeamStream: this decoder's search for num_streams streams that arrive chunk by chunk, up to max_frames frames each
        (the node pool costs 12 * beam_width bytes per frame and stream).  endpoint: an Endpointer cuts every stream into segments
        of at most endpoint.max_segment <= max_frames frames (EndpointedBeamStream), so the stream itself has no bound; every
        finished segment keeps its best `nbest` beams.  confidence: a Confidence makes the stream keep its frames on the device
        ((num_streams, max_frames, len(labels)) fp32: 4 * len(labels) bytes per frame and stream) and gives it ``words()`` and
        ``best_words()``; without it no store exists and no kernel is added to a feed.  With an endpoint the store is a ring of
        ring_capacity(endpoint) frames per stream, every finished segment comes back with ``.hypotheses`` (its kept beams'
        words, frames absolute) and ``.confidence``, and ``words()`` / ``best_words()`` give the open segment's partial."""
        if endpoint is not None:
            return EndpointedBeamStream(self, num_streams, max_frames, device, endpoint, nbest, confidence)
        return BeamStream(self, num_streams, max_frames, device, confidence)


class BeamStream:
    """Resumable beam search (ds2_beam_stream_*): after any sequence of feeds, ``result()`` equals ``decode_beams`` on the frames
    consumed so far, bit for bit.  The beam state and the node pool stay on the device; a feed does not wait for it (its host
    sizes reach the device through pinned memory in a queued copy; a host ``probs`` is copied first, which does wait).
    ``frames[n]`` counts the frames that stream n has consumed."""

    def __init__(self, decoder, num_streams, max_frames, device="cuda", confidence=None):
        d = self.decoder = decoder
        self.num_streams, self.max_frames = int(num_streams), int(max_frames)
        self.confidence, self._wc = _conf_settings(decoder, confidence)
        dev = torch.empty(0, device=device).device
        self._h = ops.beam_stream_open(self.num_streams, self.max_frames, len(d.labels), d.blank_index, d.beam_width,
                                       d.cutoff_top_n, d.cutoff_prob, dev, d._lm_args(dev), d._hot_args(dev))
        self.frames = [0] * self.num_streams
        self._store = None
        if confidence is not None:
            self._store = ops.frame_store_open(self.num_streams, self.max_frames, len(d.labels), self._h.device)

    def feed(self, probs, sizes=None):
        """probs: (N, Tc, C) probabilities of the next chunk (device or host tensor); sizes: host ints per stream (None = Tc), 0
        leaving a stream as it is.  ValueError, before anything is launched, when a stream would pass max_frames."""
        sz = _stream_sizes(sizes, self.num_streams, probs.shape[1])
        for n, v in enumerate(sz):
            if self.frames[n] + v > self.max_frames:
                raise ValueError("stream %d: %d frames consumed + %d fed pass max_frames=%d"
                                 % (n, self.frames[n], v, self.max_frames))
        if not probs.is_cuda:
            probs = probs.to(self._h.device)
        if self._store is not None and probs.shape[1]:
            x = probs if probs.dtype == torch.float32 else probs.float()
            szd = None if sizes is None else ops._sizes_to_device(sz, self._h.device)
            ops.frame_store_append(self._store, x if x.stride(2) == 1 else x.contiguous(), szd)
            ops.beam_stream_feed(self._h, x, szd)
        else:
            ops.beam_stream_feed(self._h, probs, None if sizes is None else torch.tensor(sz, dtype=torch.int32))
        self.frames = [f + v for f, v in zip(self.frames, sz)]

    def words(self, nbest=1, frame_seconds=None):
        """[[Hypothesis] * nbest] per stream (confidence.py): BeamCTCDecoder.decode_words on the frames consumed so far, bit for
        bit.  Needs a stream opened with confidence=; feeding can go on afterwards."""
        if self._store is None:
            raise ValueError("words() needs a stream opened with confidence=")
        if not 1 <= int(nbest) <= self.decoder.beam_width:
            raise ValueError("nbest must be in [1, beam_width=%d], got %r" % (self.decoder.beam_width, nbest))
        labels, _, res, scores, acoustic = ops.beam_stream_words(self._h, self._store, max(self.frames),
                                                                 dict(self._wc, nbest=int(nbest)))
        return _hypotheses(self.decoder, labels, res, scores, acoustic, frame_seconds)

    def best_words(self, frame_seconds=None):
        """The top beam's Hypothesis of every stream; only rank 0 travels to the host."""
        return [h[0] for h in self.words(1, frame_seconds)]

    def _strings(self, res):
        d = self.decoder
        strings = [[''.join(d.int_to_char[v] for v in t) for t in beams] for beams in res[0]]
        return strings, [[o.to(torch.int) for o in beams] for beams in res[1]], res[2]

    def result(self):
        """(strings, offsets, scores) in decode_beams' shapes, for the frames consumed so far; feeding can go on afterwards."""
        return self._strings(ops.beam_stream_result(self._h, max(self.frames)))

    def best(self):
        """The top beam alone: (strings[n], offsets[n]) of every stream; only rank 0 travels to the host."""
        strings, offsets, _ = self._strings(ops.beam_stream_result(self._h, max(self.frames), top_only=True))
        return [s[0] for s in strings], [o[0] for o in offsets]

    def reset(self, streams=None):
        """Streams `streams` (None = all) start again from the empty beam."""
        streams = list(range(self.num_streams)) if streams is None else [int(n) for n in streams]
        ops.beam_stream_reset(self._h, streams)
        if self._store is not None:
            ops.frame_store_reset(self._store, streams)
        for n in streams:
            self.frames[n] = 0


class EndpointedBeamStream(BeamStream):
    """A BeamStream that an Endpointer cuts into segments on the device (ops.endpoint_beam_feed): when a
    stream's segment ends, its best ``nbest`` beams -- what ``decode_beams`` gives on the segment's frames alone, bit for bit,
    the end-of-utterance terms of a language model or of hot words included -- are kept on the device and the search starts again,
    so a stream runs for any length on a node pool of max_frames >= endpoint.max_segment frames and ``feed`` never refuses for
    length.  A feed waits for nothing; ``best()`` / ``result()`` give the OPEN segment's beams, ``segments()`` drains the finished
    ones, and both fetch what has ended in between.  The device keeps at most RING_SLOTS finished segments per stream: after that
    many device feeds without a fetch, the feed fetches (the one host wait that feeding can take; a chunk longer than
    endpoint.sub_feed frames is several device feeds).  Offsets are absolute stream frames; ``frames[n]`` counts all frames."""

    RING_SLOTS = RING_SLOTS

    def __init__(self, decoder, num_streams, max_frames, device, endpoint, nbest=1, confidence=None):
        endpoint.check_max_frames(max_frames)
        super().__init__(decoder, num_streams, max_frames, device)
        self.confidence, self._wc = _conf_settings(decoder, confidence)
        if confidence is not None:
            self._store = ops.frame_store_open(self.num_streams, ring_capacity(endpoint, self.RING_SLOTS), len(decoder.labels),
                                               self._h.device)
        e = self.endpoint = endpoint
        self.nbest = int(nbest)
        self._ep = ops.endpoint_open(self.num_streams, decoder.blank_index, e.blank_threshold, e.min_trailing, e.max_leading,
                                     e.max_segment, self._h.device)
        self._sink = ops.endpoint_sink_open(self._h, self.nbest, e.max_segment, self.RING_SLOTS)
        self._done, self._since = [[] for _ in range(self.num_streams)], 0

    def feed(self, probs, sizes=None):
        """BeamStream.feed without the bound: a chunk longer than endpoint.sub_feed frames is fed in pieces, each of which can
        end at most one segment per stream."""
        sz = _stream_sizes(sizes, self.num_streams, probs.shape[1])
        if not probs.is_cuda:
            probs = probs.to(self._h.device)
        if probs.dtype != torch.float32:
            probs = probs.float()
        if self._store is not None and probs.stride(2) != 1:
            probs = probs.contiguous()
        for t0, t1, sub in split_feed(sz, self.endpoint.sub_feed):
            if self._store is not None:
                szd = ops._sizes_to_device(sub, self._h.device)
                ops.frame_store_append(self._store, probs[:, t0:t1], szd)
                ops.endpoint_beam_feed(self._ep, self._h, self._sink, probs[:, t0:t1], szd)
            else:
                ops.endpoint_beam_feed(self._ep, self._h, self._sink, probs[:, t0:t1], torch.tensor(sub, dtype=torch.int32))
            self._fed_once()
        self.frames = [f + v for f, v in zip(self.frames, sz)]

    def _fed_once(self):
        self._since += 1
        if self._since >= self.RING_SLOTS:       # a ring may be full: fetch before the next segment can end
            self._fetch()

    def _fetch(self):
        d = self.decoder
        fetched = ops.endpoint_sink_fetch(self._sink)
        hyp = self._segment_hypotheses(fetched) if self._store is not None else None
        for n, segs in enumerate(fetched):
            for k, s in enumerate(segs):
                seg = Segment(s["index"], s["start"], s["end"], s["reason"],
                              [''.join(d.int_to_char[v] for v in t) for t in s["labels"]],
                              [o.to(torch.int) + s["start"] for o in s["offsets"]], s["scores"], s["acoustic"], s["labels"])
                self._done[n].append(seg if hyp is None else WordSegment(seg, hyp[n][k]))
        self._since = 0

    def _segment_hypotheses(self, fetched):
        """[n][k]: the Hypothesis list of stream n's k-th fetched segment.  All of them go up in one copy; the k-th segments of
        all streams share one pass over the ring."""
        N, R = self.num_streams, self.nbest
        out = [[None] * len(segs) for segs in fetched]
        groups = []
        for k in range(max(len(segs) for segs in fetched)):
            sizes, starts, hyps = [0] * N, [0] * N, [[([], [])] * R for _ in range(N)]
            for n, segs in enumerate(fetched):
                if k < len(segs):
                    s = segs[k]
                    sizes[n], starts[n] = s["end"] - s["start"] + 1, s["start"]
                    hyps[n] = [(t, o.tolist()) for t, o in zip(s["labels"], s["offsets"])]
            groups.append((sizes, starts, hyps))
        if not groups:
            return out
        for k, (labels, _, res) in enumerate(ops.ring_segments_words(self._store, groups, self.decoder.blank_index, self._wc)):
            sc = [None if k >= len(segs) else (segs[k]["scores"], segs[k]["acoustic"]) for segs in fetched]
            hy = _hypotheses(self.decoder, labels, res, shifts=groups[k][1])
            for n, segs in enumerate(fetched):
                if k < len(segs):
                    out[n][k] = [h._replace(score=float(sc[n][0][r]), acoustic=float(sc[n][1][r])) for r, h in enumerate(hy[n])]
        return out

    def words(self, nbest=1, frame_seconds=None):
        """[[Hypothesis] * nbest] per stream for the OPEN segment's beams (frames absolute): BeamCTCDecoder.decode_words on the
        open segment's frames.  Finished segments carry theirs (``Segment.hypotheses``)."""
        if self._store is None:
            raise ValueError("words() needs a stream opened with confidence=")
        if not 1 <= int(nbest) <= self.decoder.beam_width:
            raise ValueError("nbest must be in [1, beam_width=%d], got %r" % (self.decoder.beam_width, nbest))
        st = self._ep.state
        labels, _, res, scores, acoustic = ops.beam_stream_words(
            self._h, self._store, min(max(self.frames), self.endpoint.max_segment), dict(self._wc, nbest=int(nbest)),
            st[:, 3] - st[:, 0], st[:, 0] % self._store.cap)
        starts = ops.endpoint_state(self._ep)[:, 0].tolist()
        return _hypotheses(self.decoder, labels, res, scores, acoustic, frame_seconds, starts)

    def _open_beams(self, top_only):
        res = ops.beam_stream_result(self._h, min(max(self.frames), self.endpoint.max_segment), top_only=top_only)
        start = ops.endpoint_state(self._ep)[:, 0].tolist()
        self._fetch()
        strings, offsets, scores = self._strings(res)
        return strings, [[o + start[n] for o in beams] for n, beams in enumerate(offsets)], scores

    def result(self):
        """(strings, offsets, scores) in decode_beams' shapes for the open segment of every stream."""
        return self._open_beams(False)

    def best(self):
        """The top beam of every stream's open segment (the partial): (strings[n], offsets[n])."""
        strings, offsets, _ = self._open_beams(True)
        return [s[0] for s in strings], [o[0] for o in offsets]

    def end(self, streams=None):
        """The open segment of streams `streams` (None = all) ends with reason "final"; it may be empty.  Feeding may go on:
        the next frame starts the next segment."""
        ops.endpoint_beam_close(self._ep, self._h, self._sink, None if streams is None else [int(n) for n in streams])
        self._fed_once()

    def segments(self):
        """Per stream the list of Segments finished since the last call, in the order they ended."""
        self._fetch()
        out, self._done = self._done, [[] for _ in range(self.num_streams)]
        return out

    def reset(self, streams=None):
        """Streams `streams` (None = all) start again: frame 0, segment 0, the empty beam; their undrained segments are dropped."""
        self._fetch()
        streams = list(range(self.num_streams)) if streams is None else [int(n) for n in streams]
        super().reset(streams)
        ops.endpoint_reset(self._ep, streams)
        for n in streams:
            self._done[n] = []


def _edit_distance(a, b):
    try:
        import Levenshtein as Lev
        return Lev.distance(a, b)
    except Exception:
        prev = list(range(len(b) + 1))
        for i, ca in enumerate(a, 1):
            cur = [i]
            for j, cb in enumerate(b, 1):
                cur.append(min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (ca != cb)))
            prev = cur
        return prev[-1]


class _ErrorRate:
    """validation.py:13-45 without torchmetrics (single process; Lightning's DDP metric sync needs the reference class)."""

    def __init__(self, decoder, target_decoder):
        self.decoder, self.target_decoder = decoder, target_decoder
        self.errors, self.total = 0, 0

    def __call__(self, preds, preds_sizes, targets, target_sizes):
        return self.update(preds, preds_sizes, targets, target_sizes)

    def update(self, preds, preds_sizes, targets, target_sizes):
        split_targets, offset = [], 0
        for size in target_sizes:
            split_targets.append(targets[offset:offset + int(size)])
            offset += int(size)
        decoded_output, _ = self.decoder.decode(preds, preds_sizes)
        target_strings = self.target_decoder.convert_to_strings(split_targets)
        for x in range(len(target_strings)):
            self.calculate_metric(decoded_output[x][0], target_strings[x][0])

    def compute(self):
        return float(self.errors) / max(self.total, 1) * 100

    def reset(self):
        self.errors, self.total = 0, 0


class CharErrorRate(_ErrorRate):   # validation.py:48-87
    def calculate_metric(self, transcript, reference):
        self.errors += _edit_distance(transcript.replace(' ', ''), reference.replace(' ', ''))
        self.total += len(reference.replace(' ', ''))


class WordErrorRate(_ErrorRate):   # validation.py:90-132
    def calculate_metric(self, transcript, reference):
        b = set(transcript.split() + reference.split())
        word2char = dict(zip(b, range(len(b))))
        w1 = ''.join(chr(word2char[w]) for w in transcript.split())
        w2 = ''.join(chr(word2char[w]) for w in reference.split())
        self.errors += _edit_distance(w1, w2)
        self.total += len(reference.split())
