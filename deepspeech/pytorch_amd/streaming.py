"""Chunked inference with text while the audio arrives: the device counterpart of the reference's ``run_transcribe`` loop
(inference.py:79-99: eval mode, ``hs`` fed back chunk after chunk, every chunk's output moved to the host, one decode after the
last chunk), for N >= 1 streams that advance in lock step.

A ``StreamingTranscriber`` carries the model's hidden state together with a decoder stream (decoder.BeamStream or
decoder.GreedyStream).  Every feed runs the model on the chunk, hands the chunk's probabilities to the decoder stream on the
device, and returns the best transcript so far; nothing but the surviving labels travels to the host and nothing grows with the
length of the audio except the beam search's node pool (12 * beam_width bytes per output frame and stream).  The transcript after
any feed is exactly what ``decoder.decode`` gives on the concatenation of the chunks' outputs.

A session feed waits for the device once per chunk, where it fetches the text: ``best()`` after a beam feed (the lengths, then
the labels of rank 0), the new labels in a greedy feed.  The decoder feed itself does not wait: ``forward`` returns the output
lengths as a host tensor, so reading them costs no synchronisation, and they reach the device through pinned memory.

By default the acoustic side is the reference's: the convolutions and the lookahead see each chunk on its own (every chunk
boundary is an utterance boundary to them), and ``feed_wave`` normalises every chunk's spectrogram on its own (the reference's
ChunkSpectrogramParser).

``carry_context=True`` makes the acoustic side exact as well, for uni-directional models: the conv front-end and the lookahead
carry their time context from feed to feed on the device (csrc/ds2_stream.hip), so the probabilities emitted over all feeds,
concatenated per stream, are the one-shot eval ``forward`` of the whole utterance up to floating-point summation details.  A
frame is emitted once nothing that a later feed brings can change it (``plan_feed``): with lookahead context C the first output
arrives after 2 * C + 14 input frames (``latency_frames``; 54 frames = 0.54 s at C = 20) -- the model's latency, not the
implementation's.  Streams start and end together; the last feed (``final=True``, or ``end()``) may be ragged.  ``feed_wave`` takes
raw audio in this mode too: the front-end's running normalisation is causal (``SpectrogramFrontEnd(normalize="running")``,
DESIGN.md section 3.6.4) and its streaming form gives the one-shot spectrogram's frames bit for bit however the audio is cut.

``StreamPool`` is the exact mode for streams that start and end on their own: every stream has a slot with its own frame counter
and plan, and a feed advances any subset of the open slots as one batch."""
import collections

import torch

from .decoder import BeamCTCDecoder

CONV_CARRY = 10          # frames both convolutions carry: their kernel width in time minus one

StreamPlan = collections.namedtuple("StreamPlan", "j1_old j1_new j2_old j2_new j3_old j3_new off1 off2 off3 k_in k_act k_la")


def _range_ends(G, ctx, final):
    """How many conv1 / conv2 (= RNN) / output frames are final after G input frames of a stream"""
    if final:
        Tp = (G - 1) // 2 + 1 if G > 0 else 0
        return Tp, Tp, Tp
    J1 = 0 if G < 6 else (G - 6) // 2 + 1          # conv1 frame j reads inputs 2j-5 .. 2j+5
    J2 = max(J1 - 5, 0)                             # conv2 frame j reads conv1 activations j-5 .. j+5
    return J1, J2, max(J2 - (ctx - 1), 0)           # output t reads RNN rows t .. t+ctx-1


def plan_feed(frames, chunk, ctx, final=False):
    """ds2_stream_plan: after `frames` input frames, a feed of `chunk` more computes conv1 frames [j1_old, j1_new), conv2 and RNN
    frames [j2_old, j2_new) and outputs [j3_old, j3_new) (global indices, any range may be empty); off1..3 are the positions of
    the first frame each kernel reads in its window [carry | chunk], k_* the carried positions."""
    frames, chunk, ctx = int(frames), int(chunk), int(ctx)
    if frames < 0 or chunk < 0 or ctx < 1:
        raise ValueError("plan_feed: frames and chunk must be >= 0 and ctx >= 1")
    o, e = _range_ends(frames, ctx, False), _range_ends(frames + chunk, ctx, bool(final))
    return StreamPlan(o[0], e[0], o[1], e[1], o[2], e[2], 2 * o[0] + 5 - frames, o[1] + 5 - o[0], o[2] + (ctx - 1) - o[1],
                      CONV_CARRY, CONV_CARRY, ctx - 1)


class StreamingTranscriber:
    def __init__(self, model, decoder, front_end=None, max_frames=6000, carry_context=False, endpoint=None, confidence=None,
                 keywords=None):
        """model: a DeepSpeech on a HIP device; decoder: a BeamCTCDecoder or GreedyDecoder over the model's labels; front_end: a
        SpectrogramFrontEnd for feed_wave (None = one with the model's spect_cfg, made on first use).  max_frames bounds the output
        frames per stream of a beam decoder (its node pool is allocated at the first feed).  carry_context: exact chunked
        inference (module docstring); uni-directional models only -- a reverse direction cannot be streamed exactly.
        endpoint: a decoder.Endpointer cuts every stream into utterances on the device: feeds return
        the partial of the open segment, ``segments()`` drains the finished ones, max_frames bounds a segment and not the stream,
        and only the decoder starts again at an endpoint -- the acoustic state runs on.
        confidence: a confidence.Confidence makes the decoder stream keep max_frames frames of probabilities per stream on the
        device and gives the session ``words()`` / ``best_words()``; with an endpoint the frames live in a ring, ``segments()``
        returns decoder.WordSegments that carry ``.hypotheses``, and ``words()`` is the open segment's partial.
        keywords: a keywords.KeywordSpotter gets every chunk's probabilities and sizes as the decoder stream does (DESIGN.md
        section 3.9); ``detections()`` drains what it found, a final feed or ``end`` emits its open candidates."""
        self.model, self.decoder, self.front_end, self.max_frames = model, decoder, front_end, int(max_frames)
        self.endpoint, self.confidence = endpoint, confidence
        self.keywords, self._kws, self._dets = keywords, None, []
        if endpoint is not None and isinstance(decoder, BeamCTCDecoder):
            endpoint.check_max_frames(self.max_frames)
        self.hs, self.stream = None, None
        self.carry_context = bool(carry_context)
        if self.carry_context and model.bidirectional:
            raise ValueError("carry_context=True needs a uni-directional model: a reverse direction cannot be streamed exactly")
        self._state = None                 # the carries (allocated at the first feed)
        self._fed, self._ended, self._text = 0, False, None
        self._wave, self._source = None, None   # exact mode: the front-end's streaming handle; what the utterance is fed with
        self.last_output = None            # exact mode: (probabilities (N, J, C), valid frames per stream) of the last feed, or None

    def _open(self, N, device):
        if isinstance(self.decoder, BeamCTCDecoder):
            self.stream = self.decoder.stream(N, self.max_frames, device, endpoint=self.endpoint, confidence=self.confidence)
        else:
            self.stream = self.decoder.stream(N, device, endpoint=self.endpoint, confidence=self.confidence,
                                              max_frames=self.max_frames if self.confidence is not None else None)
        if self.keywords is not None:
            self._kws, self._dets = self.keywords.stream(N, device), [[] for _ in range(N)]

    def _spot(self, found):
        for n, d in enumerate(found):
            self._dets[n] += d

    def detections(self):
        """keywords: per stream the list of keywords.Detections emitted since the last call, in the order they were emitted"""
        if self.keywords is None:
            raise ValueError("detections() belongs to a session with keywords=")
        out, self._dets = self._dets, [[] for _ in self._dets]
        return out

    def words(self, nbest=1, frame_seconds=None):
        """Per stream the confidence.Hypothesis list of everything fed so far, as ``decoder.decode_words`` gives it on the
        concatenation of the chunks' outputs: [[Hypothesis] * nbest] with a beam decoder, [[Hypothesis]] with a greedy one."""
        if self.confidence is None:
            raise ValueError("words() belongs to a session opened with confidence=")
        if self.stream is None:
            return []
        if isinstance(self.decoder, BeamCTCDecoder):
            return self.stream.words(nbest, frame_seconds)
        return [[h] for h in self.stream.words(frame_seconds)]

    def best_words(self, frame_seconds=None):
        """The top Hypothesis of every stream."""
        return [h[0] for h in self.words(1, frame_seconds)]

    def segments(self):
        """endpoint: per stream the list of decoder.Segments finished since the last call"""
        if self.endpoint is None:
            raise ValueError("segments() belongs to a session with an endpoint")
        return self.stream.segments() if self.stream is not None else []

    @property
    def frames(self):
        """output frames consumed per stream (host ints); with carry_context: the output frames emitted so far"""
        return list(self.stream.frames) if self.stream is not None else []

    @property
    def latency_frames(self):
        """input frames that must be fed before the first output frame: 0 without carry_context (every feed emits), else the
        smallest G with an output frame final, 2 * lookahead_context + 14"""
        if not self.carry_context:
            return 0
        return 2 * int(self.model.lookahead[0].context) + 14

    def feed(self, spect, lengths, final=False):
        """spect: (N, 1, 161, Tc) spectrogram chunk on the model's device; lengths: [N] ints, the valid input frames of every
        stream's chunk (what ``forward`` takes).  Returns the best transcript so far per stream (a list of N str).
        carry_context: every stream's length is Tc unless final=True, the last feed of the utterance, whose lengths may be ragged
        (descending, as ``forward`` takes them)."""
        m = self.model
        if self.carry_context:
            if self._source == "wave":
                raise ValueError("this utterance is fed with feed_wave; spectrogram chunks cannot be mixed in before reset()")
            self._source = "spect"
            return self._feed_exact(spect, lengths, bool(final))
        if final:
            raise ValueError("final=True is a carry_context=True feed; without it every feed stands on its own")
        if self.stream is None:
            self._open(spect.shape[0], spect.device)
        elif spect.shape[0] != self.stream.num_streams:
            raise ValueError("this session has %d streams, the chunk has %d" % (self.stream.num_streams, spect.shape[0]))
        was_training = m.training
        m.eval()
        try:
            with torch.no_grad():
                out, out_lens, self.hs = m(spect, torch.as_tensor(lengths), self.hs)
        finally:
            m.train(was_training)
        self.stream.feed(out, out_lens)                # (N, T', C) stays on the device
        if self._kws is not None:
            self._spot(self._kws.feed(out, out_lens))
        return self.best()

    def feed_wave(self, wav, nsamples, final=False):
        """wav: [N][Lmax] waveform chunk on the device, nsamples: [N] ints.  Without carry_context the chunk's spectrogram is
        computed and normalised on its own by the front end, then fed.  carry_context: the chunk goes through the front-end's
        streaming form (running normalisation, ``SpectrogramFrontEnd.stream``) and the frames it completes are fed exactly; every
        stream brings the same sample count (>= 0) unless final=True, the last feed of the utterance, whose counts may be ragged
        (descending).  A feed that completes no frame only buffers and returns the text so far."""
        if self.carry_context:
            return self._feed_wave_exact(wav, nsamples, bool(final))
        if final:
            raise ValueError("final=True is a carry_context=True feed; without it every feed stands on its own")
        if self.front_end is None:
            from .spectrogram import SpectrogramFrontEnd
            self.front_end = SpectrogramFrontEnd(getattr(self.model, "spect_cfg", None))
        inputs, _, frames = self.front_end(wav, nsamples)
        return self.feed(inputs, frames.to(torch.int))

    def _feed_wave_exact(self, wav, nsamples, final):
        if self._source == "spect":
            raise ValueError("this utterance is fed with spectrogram chunks; feed_wave cannot be mixed in before reset()")
        if self._ended:
            raise ValueError("the utterance has ended (a final feed or end()); reset() starts the next one")
        if not wav.is_cuda:
            raise ValueError("feed_wave needs the waveform chunk on the model's HIP device, got a %s tensor: the streaming front-end "
                             "has no CPU path" % wav.device)
        if self.front_end is None:
            from .spectrogram import SpectrogramFrontEnd
            self.front_end = SpectrogramFrontEnd(getattr(self.model, "spect_cfg", None), normalize="running")
        if self.front_end.normalize is True:
            raise ValueError("carry_context=True needs a causal front-end: normalize=True takes the mean and the standard deviation "
                             "of the whole utterance, which a stream does not have yet; build it with normalize='running'")
        ns = [int(v) for v in nsamples]
        N = wav.shape[0] if wav.dim() == 2 else -1
        if N < 1 or len(ns) != N:
            raise ValueError("expected a [N][L] waveform chunk and N sample counts, got %s and %s" % (tuple(wav.shape), ns))
        if not final and any(v != ns[0] for v in ns):
            raise ValueError("a feed that is not final needs the same sample count for every stream, got %s" % ns)
        if final and any(a < b for a, b in zip(ns, ns[1:])):
            raise ValueError("the final feed's sample counts must descend, got %s" % ns)
        if self._wave is None:
            self._wave = self.front_end.stream(N, wav.device)
        elif N != self._wave.capacity:
            raise ValueError("this session has %d streams, the chunk has %d" % (self._wave.capacity, N))
        spect, frames = self._wave.feed(range(N), wav, ns, final=range(N) if final else ())
        self._source = "wave"
        if not final and frames[0] == 0:
            self.last_output = None
            return list(self._text) if self._text is not None else [''] * N
        return self._feed_exact(spect, frames, final)

    def best(self):
        """the best transcript so far per stream"""
        if self.stream is None:
            return []
        if isinstance(self.decoder, BeamCTCDecoder):
            return self.stream.best()[0]
        return list(self.stream.text)

    def finish(self):
        """(strings, offsets) in ``decoder.decode``'s shapes for everything fed so far.  The session stays usable: more chunks
        may follow, and ``reset`` starts new utterances."""
        if self.stream is None:
            raise ValueError("StreamingTranscriber.finish: nothing has been fed")
        if isinstance(self.decoder, BeamCTCDecoder):
            strings, offsets, _ = self.stream.result()
            return strings, offsets
        return [[t] for t in self.stream.text], [[o] for o in self.stream.offsets]

    def reset(self):
        """Every stream starts a new utterance: the hidden state and the decoder state are dropped; with carry_context the carries
        are zeroed on the device."""
        self.hs = None
        if self.stream is not None:
            self.stream.reset()
        if self._kws is not None:
            self._kws.reset()
            self._dets = [[] for _ in self._dets]
        if self._state is not None:
            self._state["buf"].zero_()
            self._state["cur"] = [0, 0, 0]
        self._fed, self._ended, self.last_output = 0, False, None
        self._source = None
        if self._wave is not None:
            self._wave.reset()
        if self._text is not None:
            self._text = [''] * len(self._text)

    # ---- exact mode -----------------------------------------------------------------------------------------------------------
    def end(self):
        """carry_context: the end of the utterance as a final feed of nothing -- every frame still held back is emitted (after a
        ``feed_wave``: the front-end's last frame first).  Returns the transcripts."""
        if not self.carry_context:
            raise ValueError("end() belongs to carry_context=True; without it there is nothing held back")
        if self._source == "wave":
            N = self._wave.capacity
            return self._feed_wave_exact(torch.empty((N, 0), dtype=torch.float32, device=self._wave.device), [0] * N, True)
        if self._state is None:
            raise ValueError("StreamingTranscriber.end: nothing has been fed")
        N, F0 = self._state["N"], self.model._F0
        return self._feed_exact(torch.empty((N, 1, F0, 0), dtype=torch.float32, device=self._state["buf"].device), [0] * N, True)

    def _feed_exact(self, spect, lengths, final):
        from . import ops
        m = self.model
        if self._ended:
            raise ValueError("the utterance has ended (a final feed or end()); reset() starts the next one")
        if spect.dim() != 4 or spect.shape[1] != 1 or spect.shape[2] != m._F0:
            raise ValueError("expected a (N, 1, %d, Tc) spectrogram chunk, got %s" % (m._F0, tuple(spect.shape)))
        N, Tc = spect.shape[0], spect.shape[3]
        lens = [int(v) for v in lengths]
        if len(lens) != N:
            raise ValueError("%d lengths for %d streams" % (len(lens), N))
        if not final and (Tc < 1 or any(v != Tc for v in lens)):
            raise ValueError("a feed that is not final needs every stream's length to be the chunk's %d frames (>= 1), got %s" % (Tc, lens))
        if final and (any(v < 0 or v > Tc for v in lens) or any(a < b for a, b in zip(lens, lens[1:]))):
            raise ValueError("the final feed's lengths must lie in [0, %d] and descend, got %s" % (Tc, lens))
        if self.stream is None:
            self._open(N, spect.device)
            self._text = [''] * N
        elif N != self.stream.num_streams:
            raise ValueError("this session has %d streams, the chunk has %d" % (self.stream.num_streams, N))
        ctx, H, dev = int(m.lookahead[0].context), m._Hp, spect.device
        dtype = m._stream_begin()
        st = self._state
        if st is None or st["dtype"] != dtype:
            cin, cact, cla, buf = ops.stream_state_views(dtype, N, m._F0, H, ctx, dev)
            st = self._state = dict(cin=cin, cact=cact, cla=cla, buf=buf, cur=[0, 0, 0], N=N, dtype=dtype)
        chunk = max(lens) if lens else 0
        p = plan_feed(self._fed, chunk, ctx, final)
        J1, J2, J3 = p.j1_new - p.j1_old, p.j2_new - p.j2_old, p.j3_new - p.j3_old
        len_dev = live1 = live2 = None
        sizes = [J3] * N
        if final:
            # the streams' own ends: inputs, activations and RNN rows beyond them read as zero, masked frames are written as zero
            tot = [(self._fed + v - 1) // 2 + 1 if self._fed + v > 0 else 0 for v in lens]
            sizes = [min(max(t - p.j3_old, 0), J3) for t in tot]
            host = torch.tensor([lens, [min(max(t - p.j1_old, 0), J1) for t in tot], [min(max(t - p.j2_old, 0), J2) for t in tot]],
                                dtype=torch.int32)
            len_dev, live1, live2 = host.to(dev, non_blocking=True)
        x = spect.contiguous().float()
        self.last_output = None
        with torch.no_grad():
            w1k, b1, s1, h1, w2t, b2, s2, h2 = m.stream_front_weights(dtype)
            cur = st["cur"]
            a1 = None
            if chunk > 0 or J1 > 0:
                a1 = ops.stream_conv1(x, st["cin"][cur[0]], st["cin"][1 - cur[0]], w1k, b1, s1, h1, p.off1, J1, dtype, lens=len_dev, live=live1)
                cur[0] ^= 1
            if J1 > 0 or J2 > 0:
                if a1 is None:
                    a1 = torch.empty((N, m._F1, 0, 32), dtype=dtype, device=dev)
                x0 = ops.stream_conv2(a1, st["cact"][cur[1]], st["cact"][1 - cur[1]], w2t, b2, s2, h2, p.off2, J2, m._rnn_ld, F0=m._F0,
                                      live=live2)
                cur[1] ^= 1
            if J2 > 0:
                rnn_lens = live2 if final else torch.full((N,), J2, dtype=torch.int32, device=dev)
                rows, self.hs = m.stream_rnn(x0, rnn_lens, N, J2, self.hs)
                y = ops.stream_lookahead(rows, st["cla"][cur[2]], st["cla"][1 - cur[2]], m.stream_lookahead_weight(), N, H, p.off3, J3)
                if ctx > 1:
                    cur[2] ^= 1
                if J3 > 0:
                    probs = m.stream_head(y, N, J3)
                    self.last_output = (probs, sizes)
                    self.stream.feed(probs, torch.tensor(sizes, dtype=torch.int))
                    if self._kws is not None:
                        self._spot(self._kws.feed(probs, torch.tensor(sizes, dtype=torch.int)))
                    self._text = self.best()
        if final and self._kws is not None:
            self._spot(self._kws.end())
        if final and self.endpoint is not None:
            self.stream.end()                      # the last segment closes; the open one is empty from here on
            self._text = [''] * N
        self._fed += chunk
        self._ended = final
        return list(self._text)


# ---- a pool of streams that start and end on their own ----------------------------------------------
RowPlan = collections.namedtuple("RowPlan", "plans off1 off2 off3 cnt1 cnt2 cnt3 J1 J2 J3 order n_rnn")


def plan_rows(fed, lens, finals, ctx):
    """One feed of streams that each follow their own plan.  Per row r: fed[r] input frames so far, a chunk of lens[r] >= 0 more,
    finals[r] whether the utterance ends with it.  Returns per row plans[r] = plan_feed(fed[r], lens[r], ctx, finals[r]), its
    window offsets off1..3 and the counts cnt1..3 = j*_new - j*_old; for the launch the maxima J1..3 of the counts, `order` (the
    rows sorted by cnt2 descending, stable: what the recurrent stack takes) and n_rnn, the rows with cnt2 > 0 -- a prefix of
    `order`; only they run the recurrent stack, the lookahead and the head."""
    if not len(fed) == len(lens) == len(finals):
        raise ValueError("plan_rows: %d / %d / %d entries" % (len(fed), len(lens), len(finals)))
    plans = [plan_feed(g, c, ctx, f) for g, c, f in zip(fed, lens, finals)]
    cnt = [[p.j1_new - p.j1_old for p in plans], [p.j2_new - p.j2_old for p in plans], [p.j3_new - p.j3_old for p in plans]]
    assert all(c2 > 0 or c3 == 0 for c2, c3 in zip(cnt[1], cnt[2]))          # an output frame needs an RNN frame of the same feed
    order = sorted(range(len(plans)), key=lambda r: -cnt[1][r])               # sorted() is stable
    J = [max(c, default=0) for c in cnt]
    return RowPlan(plans, [p.off1 for p in plans], [p.off2 for p in plans], [p.off3 for p in plans], cnt[0], cnt[1], cnt[2],
                   J[0], J[1], J[2], order, sum(c > 0 for c in cnt[1]))


class StreamPool:
    """Exact chunked inference (``StreamingTranscriber(carry_context=True)``'s guarantee) for up to `capacity` streams that join,
    advance and end whenever their callers do.  Every stream has a slot: its carries, its hidden state, its decoder stream and its
    own frame counter.  A feed serves any subset of the open slots with chunks of any lengths as ONE batch -- one conv1, one conv2,
    one recurrent stack over the rows that retire an RNN frame, one lookahead, one head, one decoder feed -- and per stream the
    probabilities emitted over its feeds, concatenated, are the one-shot eval ``forward`` of that utterance alone."""

    def __init__(self, model, decoder, capacity, max_frames=6000, front_end=None, endpoint=None, confidence=None, keywords=None):
        """model: a uni-directional DeepSpeech on a HIP device (run in eval mode, no autograd); decoder: a BeamCTCDecoder or
        GreedyDecoder over its labels; max_frames bounds the output frames per stream of a beam decoder; front_end: a causal
        SpectrogramFrontEnd for feed_wave (None = one with the model's spect_cfg and normalize="running", made on first use).
        endpoint: a decoder.Endpointer cuts every slot's stream into utterances on the device: feeds
        return the partial of the open segment, ``segments(slot)`` drains the finished ones, a final feed or ``end`` closes the
        last one, max_frames bounds a segment and not the stream, and the acoustic state is not reset at an endpoint.
        confidence: a confidence.Confidence makes the decoder stream keep max_frames frames of probabilities per slot on the
        device and gives the pool ``words(slot)``; with an endpoint the frames live in a ring, ``segments(slot)`` returns
        decoder.WordSegments that carry ``.hypotheses``, and ``words(slot)`` is the open segment's partial.
        keywords: a keywords.KeywordSpotter gets the block and the sizes of every feed as the decoder stream does (DESIGN.md
        section 3.9); ``detections(slot)`` drains what it found in the slot's stream, ``open`` resets the slot's keyword state, a
        final feed or ``end`` emits the slot's open candidates."""
        if model.bidirectional:
            raise ValueError("a StreamPool needs a uni-directional model: a reverse direction cannot be streamed exactly")
        if int(capacity) < 1:
            raise ValueError("capacity must be >= 1, got %s" % (capacity,))
        self.model, self.decoder, self.capacity, self.max_frames = model, decoder, int(capacity), int(max_frames)
        self.endpoint, self.confidence = endpoint, confidence
        if endpoint is not None and isinstance(decoder, BeamCTCDecoder):
            endpoint.check_max_frames(self.max_frames)
        S = self.capacity
        self._segs = [[] for _ in range(S)]                # endpoint: per slot the finished segments not yet handed out
        self.keywords, self._kws = keywords, None
        self._dets = [[] for _ in range(S)]                # keywords: per slot the detections not yet handed out
        self.stream, self._state, self._h = None, None, None
        self._open = [False] * S
        self._fed, self._ended, self._text = [0] * S, [False] * S, [''] * S
        self._cur, self._fresh = [0] * S, [7] * S          # per slot, bit s - 1: stage s's carry buffer / its carry reads as zero
        self._h_zero = [True] * S                          # the slot's hidden state is the zero state of a new stream
        self.front_end, self._wave = front_end, None       # feed_wave: the front-end and its streaming handle over the S slots
        self._source = [None] * S                          # per slot: "spect" or "wave", what its stream is fed with
        self._rate = [None] * S                            # per slot: its stream's sample rate, for a front-end with a set of rates
        self.last_output = {}                              # slot -> (cnt3, C) probabilities of the last feed that held the slot

    # ---- slots ------------------------------------------------------------------------------------------------------------------
    def open(self, rate=None):
        """A free slot with fresh state: zero hidden state, carries that read as zero, a reset decoder stream, no frames fed.
        rate: the sample rate in Hz of the stream that starts, one of the front-end's ``input_rate`` set -- required when the
        front-end was built with a set of rates, refused otherwise."""
        rates = getattr(self.front_end, "rates", None)
        if rates is None and rate is not None:
            raise ValueError("open(rate=%r): the pool's front-end has one input rate; build it with input_rate=(...) for a rate "
                             "per stream" % (rate,))
        if rates is not None and (rate is None or int(rate) != rate or int(rate) not in rates):
            raise ValueError("the pool's front-end takes the rates %r: open(rate=...) must name one of them, got %r" % (rates, rate))
        if all(self._open):
            raise ValueError("the pool is full: all %d slots are open" % self.capacity)
        s = self._open.index(False)
        self._rate[s] = None if rate is None else int(rate)
        self._open[s] = True
        self._fed[s], self._ended[s], self._text[s], self._fresh[s] = 0, False, '', 7
        self._source[s] = None
        if self._wave is not None:
            self._wave.reset([s]) if rate is None else self._wave.reset([s], rates=[int(rate)])
        self.last_output.pop(s, None)
        if self.stream is not None:
            if self.endpoint is not None:
                self._pull_segments()
            self.stream.reset([s])
        if self._kws is not None:
            self._kws.reset([s])
        self._dets[s] = []
        self._segs[s] = []
        if self._h is not None and not self._h_zero[s]:
            self._h[:, :, s].zero_()
        self._h_zero[s] = True
        return s

    def close(self, slot):
        """Frees the slot for the next ``open``."""
        self._check_slots([slot])
        self._open[int(slot)] = False

    def _pull_segments(self):
        for n, segs in enumerate(self.stream.segments()):
            self._segs[n] += segs

    def segments(self, slot):
        """endpoint: the decoder.Segments of the slot's stream finished since the last call"""
        s = self._check_slots([slot])[0]
        if self.endpoint is None:
            raise ValueError("segments() belongs to a pool with an endpoint")
        if self.stream is not None:
            self._pull_segments()
        out, self._segs[s] = self._segs[s], []
        return out

    def detections(self, slot):
        """keywords: the keywords.Detections of the slot's stream emitted since the last call, in the order they were emitted"""
        s = self._check_slots([slot])[0]
        if self.keywords is None:
            raise ValueError("detections() belongs to a pool with keywords=")
        out, self._dets[s] = self._dets[s], []
        return out

    def frames(self, slot):
        """output frames emitted so far for the slot's stream"""
        self._check_slots([slot])
        return self.stream.frames[int(slot)] if self.stream is not None else 0

    @property
    def latency_frames(self):
        """input frames a stream must be fed before its first output frame: 2 * lookahead_context + 14"""
        return 2 * int(self.model.lookahead[0].context) + 14

    def _check_slots(self, slots):
        sl = [int(s) for s in slots]
        for s in sl:
            if not 0 <= s < self.capacity or not self._open[s]:
                raise ValueError("slot %d is not an open slot of this pool" % s)
        if len(set(sl)) != len(sl):
            raise ValueError("a slot appears twice: %s" % sl)
        return sl

    def finish(self, slot):
        """(strings, offsets) of the slot's stream in the shape of one entry of ``decoder.decode``, for everything emitted so far"""
        s = self._check_slots([slot])[0]
        if self.stream is None or self.stream.frames[s] == 0:
            return [''], [torch.zeros(0, dtype=torch.int)]
        if isinstance(self.decoder, BeamCTCDecoder):
            strings, offsets, _ = self.stream.result()
            return strings[s], offsets[s]
        return [self.stream.text[s]], [self.stream.offsets[s]]

    def words(self, slot, nbest=1, frame_seconds=None):
        """[Hypothesis] * nbest (confidence.py) of the slot's stream for everything emitted so far, as ``decoder.decode_words``
        gives it on the probabilities the slot's stream produced (one Hypothesis with a greedy decoder)."""
        s = self._check_slots([slot])[0]
        if self.confidence is None:
            raise ValueError("words() belongs to a pool opened with confidence=")
        if self.stream is None:                            # nothing fed yet: decode_words on no frames
            from .confidence import Hypothesis
            if not isinstance(self.decoder, BeamCTCDecoder):
                return [Hypothesis('', None, None, None, [], [], [])]
            if not 1 <= int(nbest) <= self.decoder.beam_width:
                raise ValueError("nbest must be in [1, beam_width=%d], got %r" % (self.decoder.beam_width, nbest))
            return [Hypothesis('', 0.0 if r == 0 else float("inf"), 0.0 if r == 0 else float("inf"), None, [], [], [])
                    for r in range(int(nbest))]
        if isinstance(self.decoder, BeamCTCDecoder):
            return self.stream.words(nbest, frame_seconds)[s]
        return [self.stream.words(frame_seconds)[s]]

    def end(self, slots):
        """The end of these streams' utterances as a final feed of nothing: every frame still held back is emitted (for a slot
        fed with ``feed_wave``: the front-end's last frame first)."""
        sl = self._check_slots(slots)
        dev = next(self.model.parameters()).device
        wave = [s for s in sl if self._source[s] == "wave"]
        rest = [s for s in sl if self._source[s] != "wave"]
        text = {}
        if wave:
            text.update(zip(wave, self.feed_wave(wave, torch.empty((len(wave), 0), dtype=torch.float32, device=dev), [0] * len(wave), final=wave)))
        if rest:
            text.update(zip(rest, self.feed(rest, torch.empty((len(rest), 1, self.model._F0, 0), dtype=torch.float32, device=dev),
                                            [0] * len(rest), final=rest)))
        return [text[s] for s in sl]

    def feed_wave(self, slots, wav, nsamples, final=()):
        """wav: [len(slots)][L] waveform chunks on the model's device, row i = the nsamples[i] >= 0 new samples of slots[i] (any
        counts, 0 included); final: the slots whose utterance ends with this chunk.  The chunks go through the front-end's
        streaming form (``SpectrogramFrontEnd.stream``, running normalisation) and the frames they complete are fed as ``feed``
        feeds them.  Returns the transcript so far of every slot in `slots`."""
        sl = self._check_slots(slots)
        fin = self._check_slots(final)
        for s in sl:
            if self._source[s] == "spect":
                raise ValueError("slot %d is fed with spectrogram chunks; feed_wave cannot be mixed in" % s)
            if self._ended[s]:
                raise ValueError("the stream of slot %d has ended (a final feed or end()); close() it and open() the next one" % s)
        if not sl:
            return []
        if self.front_end is None:
            from .spectrogram import SpectrogramFrontEnd
            self.front_end = SpectrogramFrontEnd(getattr(self.model, "spect_cfg", None), normalize="running")
        if self.front_end.normalize is True:
            raise ValueError("a StreamPool needs a causal front-end: normalize=True takes the mean and the standard deviation of the "
                             "whole utterance, which a stream does not have yet; build it with normalize='running'")
        if self._wave is None:
            self._wave = self.front_end.stream(self.capacity, wav.device)
            rated = [s for s in range(self.capacity) if self._rate[s] is not None]
            if rated:
                self._wave.reset(rated, rates=[self._rate[s] for s in rated])
        spect, frames = self._wave.feed(sl, wav, nsamples, final=fin)
        for s in sl:
            self._source[s] = "wave"
        return self._feed(sl, spect, frames, fin)

    # ---- the feed ---------------------------------------------------------------------------------------------------------------
    def feed(self, slots, spect, lengths, final=()):
        """spect: (len(slots), 1, F0, Tc) spectrogram chunks on the model's device, row i for slots[i] (any order); lengths[i] in
        [0, Tc]: the valid input frames of row i; final: the slots whose utterance ends with this chunk.  Returns the transcript so
        far of every slot in `slots`, in that order.  Only the fetch of the text waits for the device."""
        for s in self._check_slots(slots):
            if self._source[s] == "wave":
                raise ValueError("slot %d is fed with feed_wave; spectrogram chunks cannot be mixed in" % s)
        text = self._feed(slots, spect, lengths, final)
        for s in slots:
            self._source[int(s)] = "spect"
        return text

    def _feed(self, slots, spect, lengths, final):
        from . import ops
        m, S = self.model, self.capacity
        sl = self._check_slots(slots)
        fin = set(self._check_slots(final))
        if not fin <= set(sl):
            raise ValueError("final names slots that are not in this feed: %s" % sorted(fin - set(sl)))
        if not sl:
            return []
        for s in sl:
            if self._ended[s]:
                raise ValueError("the stream of slot %d has ended (a final feed or end()); close() it and open() the next one" % s)
        if spect.dim() != 4 or spect.shape[0] != len(sl) or spect.shape[1] != 1 or spect.shape[2] != m._F0:
            raise ValueError("expected a (%d, 1, %d, Tc) spectrogram chunk, got %s" % (len(sl), m._F0, tuple(spect.shape)))
        Tc = spect.shape[3]
        lens = [int(v) for v in lengths]
        if len(lens) != len(sl) or any(v < 0 or v > Tc for v in lens):
            raise ValueError("lengths must be %d ints in [0, %d], got %s" % (len(sl), Tc, lens))
        ctx, H, dev = int(m.lookahead[0].context), m._Hp, spect.device
        rp = plan_rows([self._fed[s] for s in sl], lens, [s in fin for s in sl], ctx)
        beam = isinstance(self.decoder, BeamCTCDecoder)
        if beam and self.endpoint is None:
            for i, s in enumerate(sl):
                have = self.stream.frames[s] if self.stream is not None else 0
                if have + rp.cnt3[i] > self.max_frames:
                    raise ValueError("slot %d: %d frames emitted + %d more pass max_frames=%d" % (s, have, rp.cnt3[i], self.max_frames))
        if self.stream is None:
            self.stream = self.decoder.stream(S, self.max_frames, dev, endpoint=self.endpoint, confidence=self.confidence) if beam else \
                self.decoder.stream(S, dev, endpoint=self.endpoint, confidence=self.confidence,
                                    max_frames=self.max_frames if self.confidence is not None else None)
            if self.keywords is not None:
                self._kws = self.keywords.stream(S, dev)
        dtype = m._stream_begin()
        st = self._state
        if st is None or st["dtype"] != dtype:
            if st is not None and any(f != 7 for s, f in enumerate(self._fresh) if self._open[s]):
                raise ValueError("the model's compute dtype changed while streams are open")
            cin, cact, cla, buf = ops.stream_state_views(dtype, S, m._F0, H, ctx, dev)
            st = self._state = dict(cin=cin, cact=cact, cla=cla, buf=buf, dtype=dtype)
        J1, J2, J3, n_rnn, order = rp.J1, rp.J2, rp.J3, rp.n_rnn, rp.order
        run1 = max(lens) > 0 or J1 > 0                    # the stages that launch, for all rows alike (StreamingTranscriber's rule)
        run2 = J1 > 0 or J2 > 0
        run3 = J2 > 0
        table = [(sl[i], i, self._cur[sl[i]], self._fresh[sl[i]], lens[i], rp.off1[i], rp.cnt1[i], rp.off2[i], rp.cnt2[i], rp.off3[i],
                  rp.cnt3[i]) for i in order]
        x = spect.contiguous().float()
        with torch.no_grad():
            rows, rnn_lens, idx = ops.stream_rows(table, S, len(sl), Tc, dev)
            w1k, b1, s1, h1, w2t, b2, s2, h2 = m.stream_front_weights(dtype)
            a1 = probs = None
            if run1:
                a1 = ops.stream_conv1_rows(x, st["cin"], rows, w1k, b1, s1, h1, J1, dtype)
                self._advance(sl, 1)
            if run2:
                if a1 is None:
                    a1 = torch.empty((len(sl), m._F1, 0, 32), dtype=dtype, device=dev)
                x0 = ops.stream_conv2_rows(a1, st["cact"], rows, n_rnn, w2t, b2, s2, h2, J2, m._rnn_ld, F0=m._F0)
                self._advance(sl, 2)
            if run3:
                rslots = [sl[i] for i in order[:n_rnn]]
                out_rows = self._run_rnn(x0, rnn_lens[:n_rnn], idx[:n_rnn], rslots, n_rnn, J2)
                y = ops.stream_lookahead_rows(out_rows, st["cla"], rows, m.stream_lookahead_weight(), n_rnn, S, H, J3)
                if ctx > 1:
                    self._advance(rslots, 4)
                if J3 > 0:
                    probs = m.stream_head(y, n_rnn, J3)                      # (n_rnn, J3, C), rows in table order
        for i, s in enumerate(sl):
            self._fed[s] += lens[i]
            self._ended[s] = s in fin
            self.last_output.pop(s, None)
        if probs is not None:
            # the decoder streams are the pool's S slots: a slot that emitted nothing takes nothing (size 0)
            full = probs.new_zeros((S, J3, probs.shape[2]))
            full.index_copy_(0, idx[:n_rnn], probs)
            sizes = [0] * S
            for r, i in enumerate(order[:n_rnn]):
                sizes[sl[i]] = rp.cnt3[i]
                if rp.cnt3[i] > 0:
                    self.last_output[sl[i]] = probs[r, :rp.cnt3[i]]
            self.stream.feed(full, torch.tensor(sizes, dtype=torch.int))
            if self._kws is not None:
                self._spot(self._kws.feed(full, torch.tensor(sizes, dtype=torch.int)))
            text = self.stream.best()[0] if beam else self.stream.text
            for s in sl:
                self._text[s] = text[s]
        if fin and self._kws is not None:
            self._spot(self._kws.end(sorted(fin)))
        if fin and self.endpoint is not None:
            self.stream.end(sorted(fin))           # the last segment closes; the open one is empty from here on
            for s in fin:
                self._text[s] = ''
        return [self._text[s] for s in sl]

    def _spot(self, found):
        for n, d in enumerate(found):
            self._dets[n] += d

    def _advance(self, slots, bit):
        """a launched stage wrote its next carry for these slots: the other buffer holds it now, and it is no longer fresh"""
        for s in slots:
            self._cur[s] ^= bit
            self._fresh[s] &= ~bit

    def _run_rnn(self, x0, rnn_lens, idx, rslots, n_rnn, J2):
        """The recurrent stack over the n_rnn rows that retire an RNN frame: their hidden states are gathered from the pool's one
        state tensor ([layers * states][directions][S][width], fp32 as ``forward`` returns them) and scattered back."""
        m = self.model
        lstm = m._kind == "lstm"
        hs = None
        if not all(self._h_zero[s] for s in rslots):       # all new: no initial state, as the first feed of a one-shot session
            g = self._h.index_select(2, idx)
            hs = [(g[2 * l], g[2 * l + 1]) for l in range(g.shape[0] // 2)] if lstm else list(g.unbind(0))
        out_rows, new_hs = m.stream_rnn(x0, rnn_lens, n_rnn, J2, hs)
        new = torch.stack([t for pair in new_hs for t in pair] if lstm else list(new_hs))
        if self._h is None:
            self._h = new.new_zeros(new.shape[:2] + (self.capacity, new.shape[3]))
        self._h.index_copy_(2, idx, new)
        for s in rslots:
            self._h_zero[s] = False
        return out_rows
