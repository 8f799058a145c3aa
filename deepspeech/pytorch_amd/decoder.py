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

    def stream(self, num_streams, device="cuda", endpoint=None):
        """A GreedyStream: decode for num_streams streams that arrive chunk by chunk.  endpoint: an Endpointer cuts every stream
        into segments (EndpointedGreedyStream)."""
        if endpoint is not None:
            return EndpointedGreedyStream(self, num_streams, device, endpoint)
        return GreedyStream(self, num_streams, device)


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


class GreedyStream:
    """GreedyDecoder.decode on streams that arrive in chunks (ds2_greedy_stream_feed): the previous frame's arg-max and the frame
    count of every stream stay on the device, so a repeated label or a run of blanks across a chunk boundary is collapsed as in the
    whole utterance.  ``text[n]`` is the transcript so far, ``offsets[n]`` its frames, ``frames[n]`` the frames consumed."""

    def __init__(self, decoder, num_streams, device="cuda"):
        self.decoder, self.num_streams = decoder, int(num_streams)
        self._carry = torch.zeros((self.num_streams, 2), dtype=torch.int32, device=device)
        self.reset()

    def reset(self, streams=None):
        """Streams `streams` (None = all) start again."""
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
        toks, offs = ops.greedy_stream_feed(probs, None if sizes is None else torch.tensor(sz, dtype=torch.int32), d.blank_index,
                                            self._carry)
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

    def __init__(self, decoder, num_streams, device, endpoint):
        e = self.endpoint = endpoint
        self._ep = ops.endpoint_open(num_streams, decoder.blank_index, e.blank_threshold, e.min_trailing, e.max_leading,
                                     e.max_segment, device)
        self._start, self._labels = [0] * int(num_streams), [[] for _ in range(int(num_streams))]
        self._done = [[] for _ in range(int(num_streams))]
        super().__init__(decoder, num_streams, self._ep.device)

    def reset(self, streams=None):
        """Streams `streams` (None = all) start again at frame 0 and segment 0; their undrained segments are dropped."""
        super().reset(streams)
        ops.endpoint_reset(self._ep, streams)
        for n in (range(self.num_streams) if streams is None else streams):
            self._start[n], self._labels[n], self._done[n] = 0, [], []

    def _finish(self, n, reason, start, end, index):
        self._done[n].append(Segment(index, start, end, reason, [self.text[n]], [self.offsets[n]], None, None, [self._labels[n]]))
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
    list runs the entry points without hot words.  These three are keywords of this class only."""

    def __init__(self, labels, lm_path=None, alpha=0, beta=0, cutoff_top_n=40, cutoff_prob=1.0, beam_width=100,
                 num_processes=4, blank_index=0, lexicon=True, hotwords=None, hotword_weight=2.0, hot_oov_logp=-11.5):
        self.lm, self.lexicon, self._tables = None, bool(lexicon), {}
        if lm_path:
            from . import lm as _lm
            if ' ' not in labels or labels.index(' ') == blank_index:
                raise ValueError("BeamCTCDecoder: a language model needs a space label other than the blank to end words")
            self.lm = _lm.load_arpa(lm_path)     # ValueError unless it is an ARPA text file of order 1 to 5
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

    def decode_beams(self, probs, sizes=None):
        """(strings, offsets, scores): strings[n] = beam_width transcripts (best first), offsets[n] = the matching int tensors of
        frames, scores = host (N, beam_width) float tensor of -log p, with an LM -(log p + lm) (lower is better; +inf where no
        beam is alive).  The reference's run_transcribe passes out.cpu() (inference.py:96-98): a host tensor is moved over."""
        return self.decode_beams_detailed(probs, sizes)[:3]

    def _lm_tables(self, device):
        """The LM's two tables on `device`: built and uploaded on first use, then kept."""
        if device not in self._tables:
            from . import lm as _lm
            wt, gt = _lm.build_tables(self.lm, self.labels, self.blank_index, self.space_index)
            self._tables[device] = (torch.from_numpy(wt).to(device), torch.from_numpy(gt).to(device))
        return self._tables[device]

    def decode_beams_detailed(self, probs, sizes=None):
        """(strings, offsets, scores, acoustic): decode_beams' three values and the acoustic -log p of the same beams.  With an
        LM, scores = acoustic - lm (the total that ranked the beams); without one the two are equal."""
        if not probs.is_cuda:
            probs = probs.to("cuda")
        ht = self._hot_table(probs.device)
        if self.lm is None and ht is not None:
            toks, offs, scores, acoustic = ops.beam_decode_hot(probs, sizes, self.blank_index, self.beam_width, self.cutoff_top_n,
                                                               self.cutoff_prob, self.space_index, ht)
        elif self.lm is None:
            toks, offs, scores = ops.beam_decode(probs, sizes, self.blank_index, self.beam_width, self.cutoff_top_n,
                                                 self.cutoff_prob)
            acoustic = scores
        elif ht is not None:
            wt, gt = self._lm_tables(probs.device)
            toks, offs, scores, acoustic = ops.beam_decode_lm_hot(probs, sizes, self.blank_index, self.beam_width, self.cutoff_top_n,
                                                                  self.cutoff_prob, self.space_index, wt, gt, self.lm.order,
                                                                  self.lm.bos, self.alpha, self.beta, self.lexicon, ht,
                                                                  self.hot_oov_logp)
        else:
            wt, gt = self._lm_tables(probs.device)
            toks, offs, scores, acoustic = ops.beam_decode_lm(probs, sizes, self.blank_index, self.beam_width, self.cutoff_top_n,
                                                              self.cutoff_prob, self.space_index, wt, gt, self.lm.order,
                                                              self.lm.bos, self.alpha, self.beta, self.lexicon)
        strings = [[''.join(self.int_to_char[v] for v in t) for t in beams] for beams in toks]
        offsets = [[o.to(torch.int) for o in beams] for beams in offs]
        return strings, offsets, scores, acoustic

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
        wt, gt = self._lm_tables(probs.device)
        return ops.beam_decode_lm_grid(probs, sizes, self.blank_index, self.beam_width, self.cutoff_top_n, self.cutoff_prob,
                                       self.space_index, wt, gt, self.lm.order, self.lm.bos, [a for a, _ in points],
                                       [b for _, b in points], self.lexicon, max_ws_bytes)

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

    def stream(self, num_streams, max_frames, device="cuda", endpoint=None, nbest=1):
        """A BeamStream: this decoder's search for num_streams streams that arrive chunk by chunk, up to max_frames frames each
        (the node pool costs 12 * beam_width bytes per frame and stream).  endpoint: an Endpointer cuts every stream into segments
        of at most endpoint.max_segment <= max_frames frames (EndpointedBeamStream), so the stream itself has no bound; every
        finished segment keeps its best `nbest` beams."""
        if endpoint is not None:
            return EndpointedBeamStream(self, num_streams, max_frames, device, endpoint, nbest)
        return BeamStream(self, num_streams, max_frames, device)


class BeamStream:
    """Resumable beam search (ds2_beam_stream_*): after any sequence of feeds, ``result()`` equals ``decode_beams`` on the frames
    consumed so far, bit for bit.  The beam state and the node pool stay on the device; a feed does not wait for it (its host
    sizes reach the device through pinned memory in a queued copy; a host ``probs`` is copied first, which does wait).
    ``frames[n]`` counts the frames that stream n has consumed."""

    def __init__(self, decoder, num_streams, max_frames, device="cuda"):
        d = self.decoder = decoder
        self.num_streams, self.max_frames = int(num_streams), int(max_frames)
        dev = torch.empty(0, device=device).device
        lm = None
        if d.lm is not None:
            wt, gt = d._lm_tables(dev)
            lm = dict(space=d.space_index, word_table=wt, ngram_table=gt, order=d.lm.order, bos=d.lm.bos, alpha=d.alpha,
                      beta=d.beta, lexicon=d.lexicon)
        ht, hot = d._hot_table(dev), None
        if ht is not None:
            hot = dict(space=d.space_index, table=ht, oov_logp=d.hot_oov_logp)
        self._h = ops.beam_stream_open(self.num_streams, self.max_frames, len(d.labels), d.blank_index, d.beam_width,
                                       d.cutoff_top_n, d.cutoff_prob, dev, lm, hot)
        self.frames = [0] * self.num_streams

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
        ops.beam_stream_feed(self._h, probs, None if sizes is None else torch.tensor(sz, dtype=torch.int32))
        self.frames = [f + v for f, v in zip(self.frames, sz)]

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

    RING_SLOTS = 8

    def __init__(self, decoder, num_streams, max_frames, device, endpoint, nbest=1):
        endpoint.check_max_frames(max_frames)
        super().__init__(decoder, num_streams, max_frames, device)
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
        for t0, t1, sub in split_feed(sz, self.endpoint.sub_feed):
            ops.endpoint_beam_feed(self._ep, self._h, self._sink, probs[:, t0:t1], torch.tensor(sub, dtype=torch.int32))
            self._fed_once()
        self.frames = [f + v for f, v in zip(self.frames, sz)]

    def _fed_once(self):
        self._since += 1
        if self._since >= self.RING_SLOTS:       # a ring may be full: fetch before the next segment can end
            self._fetch()

    def _fetch(self):
        d = self.decoder
        for n, segs in enumerate(ops.endpoint_sink_fetch(self._sink)):
            for s in segs:
                self._done[n].append(Segment(s["index"], s["start"], s["end"], s["reason"],
                                             [''.join(d.int_to_char[v] for v in t) for t in s["labels"]],
                                             [o.to(torch.int) + s["start"] for o in s["offsets"]], s["scores"], s["acoustic"],
                                             s["labels"]))
        self._since = 0

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
