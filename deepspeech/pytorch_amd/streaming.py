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

The acoustic side is the reference's: the convolutions and the lookahead see each chunk on its own, and ``feed_wave`` normalises
every chunk's spectrogram on its own (the reference's ChunkSpectrogramParser).  Carrying their context is outside this class."""
import torch

from .decoder import BeamCTCDecoder


class StreamingTranscriber:
    def __init__(self, model, decoder, front_end=None, max_frames=6000):
        """model: a DeepSpeech on a HIP device; decoder: a BeamCTCDecoder or GreedyDecoder over the model's labels; front_end: a
        SpectrogramFrontEnd for feed_wave (None = one with the model's spect_cfg, made on first use).  max_frames bounds the output
        frames per stream of a beam decoder (its node pool is allocated at the first feed)."""
        self.model, self.decoder, self.front_end, self.max_frames = model, decoder, front_end, int(max_frames)
        self.hs, self.stream = None, None

    def _open(self, N, device):
        if isinstance(self.decoder, BeamCTCDecoder):
            self.stream = self.decoder.stream(N, self.max_frames, device)
        else:
            self.stream = self.decoder.stream(N, device)

    @property
    def frames(self):
        """output frames consumed per stream (host ints)"""
        return list(self.stream.frames) if self.stream is not None else []

    def feed(self, spect, lengths):
        """spect: (N, 1, 161, Tc) spectrogram chunk on the model's device; lengths: [N] ints, the valid input frames of every
        stream's chunk (what ``forward`` takes).  Returns the best transcript so far per stream (a list of N str)."""
        m = self.model
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
        return self.best()

    def feed_wave(self, wav, nsamples):
        """wav: [N][Lmax] waveform chunk on the device, nsamples: [N] ints.  The chunk's spectrogram is computed and normalised on
        its own by the front end, then fed."""
        if self.front_end is None:
            from .spectrogram import SpectrogramFrontEnd
            self.front_end = SpectrogramFrontEnd(getattr(self.model, "spect_cfg", None))
        inputs, _, frames = self.front_end(wav, nsamples)
        return self.feed(inputs, frames.to(torch.int))

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
        """Every stream starts a new utterance: the hidden state and the decoder state are dropped."""
        self.hs = None
        if self.stream is not None:
            self.stream.reset()
