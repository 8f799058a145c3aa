"""Device-side replacement for the CPU spectrogram workers of the reference loader: ``SpectrogramParser.compute_spectrogram``
(loader/data_loader.py:73-94) for every utterance of a batch + the zero-padded batch layout of ``_collate_fn`` (:247-270), as one
call on the HIP kernels of csrc/ds2_spect.hip.  Output = exactly the ``inputs`` / ``input_percentages`` the model's
``training_step`` takes.  Geometry: 16 kHz, 20 ms window, 10 ms stride (n_fft 320, hop 160 -> 161 bins), the geometry this
front-end's DFT GEMM is specialised for (the conv kernels take any bin count, ``ops.conv_rows``; 8 kHz / 81-bin spectrograms have
to come from elsewhere); the window type follows ``SpectConfig.window`` (enums.py:8-14).  With ``augment=True`` the reference's
``spec_augment`` (loader/spec_augment.py:68-115, see ``augment.SpecAugment``) is folded into the same call.  A front-end built with
``wave_augment=augment.WaveAugment(...)`` first runs the loader's waveform augmentations (tempo, gain, noise injection,
data_loader.py:151-159) on the device, so one call covers everything ``parse_audio`` does; with a ``rir_bank`` it also
reverberates clips between tempo and gain (``augment.RirBank``, the project's own addition).  Waveforms at another sample rate
(``input_rate=44100``, ...) are converted to 16 kHz on the device in front of all that (``resample.Resampler``, DESIGN.md section
7.2), one-shot and in ``stream()``.

The reference's STFT lives in a third-party dependency that is not vendored and not pinned (``librosa``, requirements.txt:4):
``center=True`` padding is zeros in librosa >= 0.10 (``pad_mode="constant"``, the default here) and reflection before
(``pad_mode="reflect"`` = ``np.pad(y, 160, "reflect")`` for every length >= 1: a clip shorter than the pad is folded as often as
it takes, a single sample repeats)."""
import collections
import math

import numpy as np
import torch

from . import ops
from ._lib import Ds2HipError, call, query
from .augment import SpecAugment

N_FFT, HOP, N_BIN = 320, 160, 161
_TORCH_DTYPE = {np.dtype(np.int32): torch.int32, np.dtype(np.float32): torch.float32, np.dtype(np.int64): torch.int64}


def window_values(name, n=N_FFT):
    """Periodic (fftbins=True) windows as scipy.signal.get_window / librosa.filters.get_window produce them."""
    k = np.arange(n, dtype=np.float64)
    name = getattr(name, "value", name)
    if name == "hamming":
        return 0.54 - 0.46 * np.cos(2 * np.pi * k / n)
    if name == "hann":
        return 0.5 - 0.5 * np.cos(2 * np.pi * k / n)
    if name == "blackman":
        return 0.42 - 0.5 * np.cos(2 * np.pi * k / n) + 0.08 * np.cos(4 * np.pi * k / n)
    if name == "bartlett":
        return 1.0 - np.abs(2.0 * k / n - 1.0)
    raise ValueError("unsupported spectrogram window %r" % (name,))


def dft_basis(window):
    """[2*161][320] float32: rows 0..160 = w[k] cos(2 pi f k / 320), rows 161..321 = -w[k] sin(2 pi f k / 320)."""
    w = window_values(window)
    f = np.arange(N_BIN, dtype=np.float64)[:, None]
    k = np.arange(N_FFT, dtype=np.float64)[None, :]
    ang = 2 * np.pi * f * k / N_FFT
    return np.concatenate([np.cos(ang) * w, -np.sin(ang) * w], 0).astype(np.float32)


WavePlan = collections.namedtuple("WavePlan", "frames_before emit carried window new_carry first")


def plan_wave(samples_before, n_new, final=False):
    """ds2_spect_stream_plan: after `samples_before` samples of a stream, a feed of `n_new` more (final: the utterance ends with
    it).  G samples complete G // 160 frames -- frame t covers samples [160 t - 160, 160 t + 160) -- and the end completes
    1 + G // 160, so the feed emits the difference: possibly nothing, possibly one frame from no new samples (the flush).  The
    feed's window is [carried | new | 160 zeros if final]: `carried` = 160 + samples_before % 160 samples in front of the new ones
    (the left centre padding while it is in reach), `window` its length, `new_carry` the samples behind the last emitted frame's
    hop that the next feed needs (at most 319; 0 after a final feed), `first` the clip position of the window's first sample."""
    G0, n = int(samples_before), int(n_new)
    if G0 < 0 or n < 0:
        raise ValueError("plan_wave: samples_before and n_new must be >= 0")
    f0, G1 = G0 // HOP, G0 + n
    f1 = 1 + G1 // HOP if final else G1 // HOP
    carried = HOP + G0 % HOP
    window = carried + n + (HOP if final else 0)
    return WavePlan(f0, f1 - f0, carried, window, 0 if final else window - HOP * (f1 - f0), HOP * f0 - HOP)


class SpectrogramFrontEnd:
    def __init__(self, spect_cfg=None, normalize=True, pad_mode="constant", spec_augment=None, rng=None, wave_augment=None,
                 running_floor=1e-5, running_prior=None, input_rate=None):
        """normalize: True = (x - mean) / std over the whole utterance (the reference's), False = raw log-magnitudes, "running" =
        the causal mode: frame t is normalised with the statistics of frames 0..t, which is what
        ``stream()`` can reproduce bit for bit while the audio arrives.  running_floor: the mode's lower bound of the standard
        deviation (digital silence gives zeros, not NaN); running_prior: (mean, std, frames) pseudo-counts the statistics start
        from, None = none.  spec_augment: an ``augment.SpecAugment`` (None = its defaults) used by calls with ``augment=True``; rng: the
        numpy.random.Generator its draws come from (None = a fresh default_rng()).  wave_augment: an ``augment.WaveAugment``
        (None = none) applied to the waveforms of EVERY call, as the reference's loader applies tempo / gain / noise whenever its
        configuration asks for them; its draws come from rng too, before those of SpecAugment.  input_rate: the sample rate of
        the waveforms handed in, in Hz (None or 16000 = they are at 16 kHz already and nothing is added to any call); any other
        rate is converted to 16 kHz on the device first (``resample.Resampler``), and every count this class reports -- frames,
        percentages, ``SpectStream.samples`` -- is one of the 16 kHz signal.  A tuple or list of rates (``input_rate=(8000, 16000,
        48000)``) is the SET of rates the clips may have: every call that takes waveforms then takes ``rates=[one per clip]``, and
        the batch is converted in one launch whatever it mixes (``resample.ResamplerBank``).  A wave_augment with
        ``speed_choices`` resamples too -- a clip at rate r drawn speed s is read as one recorded at r * s Hz -- so the front-end
        then builds its bank from every rate x speed product and refuses a pair whose product is no integer number of Hz or
        whose table does not fit."""
        sr = getattr(spect_cfg, "sample_rate", 16000)
        n_fft = int(sr * getattr(spect_cfg, "window_size", 0.02))
        hop = int(sr * getattr(spect_cfg, "window_stride", 0.01))
        if (n_fft, hop) != (N_FFT, HOP):
            raise ValueError("the gfx950 front-end is specialised for n_fft 320 / hop 160 (16 kHz, 20 ms, 10 ms); got %d / %d" % (n_fft, hop))
        if pad_mode not in ("constant", "reflect"):
            raise ValueError("pad_mode must be 'constant' (librosa >= 0.10) or 'reflect'")
        self.window = getattr(spect_cfg, "window", "hamming")
        if isinstance(normalize, str) and normalize != "running":
            raise ValueError("normalize must be True, False or 'running', got %r" % (normalize,))
        self.running = normalize == "running"
        self.normalize, self.reflect = "running" if self.running else bool(normalize), pad_mode == "reflect"
        self.running_floor = float(running_floor)
        if not self.running_floor > 0.0:
            raise ValueError("running_floor must be > 0, got %r" % (running_floor,))
        self.running_prior = (0.0, 0.0, 0.0) if running_prior is None else tuple(float(v) for v in running_prior)
        if len(self.running_prior) != 3 or not (self.running_prior[1] >= 0.0 and 0.0 <= self.running_prior[2] < 1e9):
            raise ValueError("running_prior must be (mean, std >= 0, frames >= 0), got %r" % (running_prior,))
        self.spec_augment = spec_augment if spec_augment is not None else SpecAugment()
        self.rng = rng if rng is not None else np.random.default_rng()
        self._basis = {}
        self.last_coef = None            # device [N][3]: the time-warp flow coefficients of the latest augmented call
        self.wave_augment = wave_augment
        self.last_wave = None            # (WaveDraws, device [N][Smax] WSOLA offsets or None) of the latest call with wave_augment
        self.resampler = None            # one input rate other than 16 kHz
        self.rates, self.bank = None, None       # a set of input rates (rates) and / or speed perturbation: every rate x speed product
        speeds = getattr(wave_augment, "speed_choices", None)
        if isinstance(input_rate, (tuple, list)):
            if not input_rate or any(int(r) != r or int(r) <= 0 for r in input_rate) or len(set(input_rate)) != len(input_rate):
                raise ValueError("input_rate as a set must hold distinct positive integer rates in Hz, got %r" % (input_rate,))
            self.rates = tuple(int(r) for r in input_rate)
        if self.rates is not None or speeds:
            from .augment import speed_rate
            from .resample import Resampler, ResamplerBank
            self._one_rate = None if self.rates is not None else int(16000 if input_rate is None else input_rate)
            products = []
            for r in (self.rates if self.rates is not None else (self._one_rate,)):
                for sp in (speeds or (1,)):
                    eff = speed_rate(r, sp)
                    try:
                        Resampler(eff)
                    except ValueError as e:
                        raise ValueError("rate %d Hz at speed %s is read as %d Hz: %s" % (r, sp, eff, e)) from None
                    if eff not in products:
                        products.append(eff)
            self.bank = ResamplerBank(products)
        elif input_rate is not None and int(input_rate) != 16000:
            from .resample import Resampler
            self.resampler = Resampler(input_rate)

    def _basis_on(self, dev):
        b = self._basis.get(dev)
        if b is None:
            b = self._basis[dev] = torch.from_numpy(dft_basis(self.window)).to(dev)
        return b

    def _row_rates(self, rates, N):
        """the input rate of each of N clips: `rates` checked against the front-end's set, or its one rate N times"""
        if self.rates is None:
            if rates is not None:
                raise ValueError("rates=... belongs to a front-end built with a set of rates (input_rate=(...)); this one has "
                                 "a single input rate")
            return [self._one_rate] * N
        if rates is None:
            raise ValueError("this front-end takes clips at the rates %r: pass rates=[one per clip]" % (self.rates,))
        rates = list(rates)
        if len(rates) != N or any(int(r) != r or int(r) not in self.rates for r in rates):
            raise ValueError("rates must hold one of %r per clip (%d clips), got %r" % (self.rates, N, rates))
        return [int(r) for r in rates]

    def __call__(self, wav, nsamples, augment=False, rates=None):
        """wav: [N][Lmax] float32 on a HIP device (row n = utterance n, zero beyond nsamples[n]); nsamples: [N] ints.
        rates: the sample rate of each row, for a front-end built with a set of rates (and only for one).
        Returns (inputs (N,1,161,Tmax) float32, input_percentages [N] float32 (CPU), frames [N] int64 (CPU)).
        augment=True: every clip goes through the reference's spec_augment with draws from self.rng (one pinned upload, nothing is
        read back; the flow coefficients used stay on the device in self.last_coef)."""
        if not wav.is_cuda:
            raise Ds2HipError("SpectrogramFrontEnd needs the waveforms on a HIP device; there is no CPU path")
        wav = wav.float().contiguous()
        N, Lmax = wav.shape
        ns = torch.as_tensor(nsamples, dtype=torch.int32).cpu()
        if ns.numel() != N or int(ns.min()) < 1:
            raise ValueError("nsamples must hold one positive sample count per waveform row")
        Lm = int(ns.max())
        if Lm > Lmax:
            raise ValueError("nsamples exceeds the waveform buffer")
        ns_dev = None
        if self.bank is not None:
            # the speed of a clip is the first draw of its augmentation and decides its class, so the draws come before the launch
            base, wd = self._row_rates(rates, N), None
            if self.wave_augment is not None and self.wave_augment.speed_choices:
                wd = self.wave_augment.draw(ns.numpy(), self.rng, rates=base)
            wav, ns_dev, ns = self.bank._run(wav, ns, base if wd is None else wd.rates.tolist())
            if wd is not None:
                return self._call_wave_augmented(wav, ns, augment, wd)
            Lm = int(ns.max())
        elif rates is not None:
            self._row_rates(rates, N)
        if self.resampler is not None:   # everything below sees the 16 kHz signal and its lengths (known on the host in closed form)
            wav, ns_dev, ns = self.resampler._run(wav, ns)
            Lm = int(ns.max())
        if self.wave_augment is not None and self.wave_augment.active:
            return self._call_wave_augmented(wav, ns, augment)
        Tmax = 1 + Lm // HOP
        out = torch.empty((N, 1, N_BIN, Tmax), dtype=torch.float32, device=wav.device)
        if ns_dev is None:
            ns_dev = ns.to(wav.device)   # held in a local until the launch is enqueued (a temporary would be freed -- and its block
            #                              possibly re-used by the basis upload -- before the kernels read it)
        frames = 1 + ns.to(torch.int64) // HOP
        if augment:
            sa = self.spec_augment
            draws = sa.draw(frames.numpy(), N_BIN, self.rng)
            warp, fmask, tmask = self.upload_draws(draws, wav.device)
            self.last_coef = torch.empty((N, 3), dtype=torch.float32, device=wav.device)
            self._launch(wav, ns_dev, N, Lm, out, (warp, sa.W, fmask, draws[1].shape[1], tmask, draws[2].shape[1], self.last_coef))
        else:
            self._launch(wav, ns_dev, N, Lm, out, None)
        pct = (frames.to(torch.float64) / float(Tmax)).to(torch.float32)      # _collate_fn: seq_length / float(max_seqlength)
        return out, pct, frames

    def _launch(self, wav, ns_dev, N, Lm, out, aug):
        """The spectrogram call in the front-end's normalisation mode.  aug: None, or (warp draws, W, frequency masks, their count
        per clip, time masks, their count, coefficients out) for the call with SpecAugment folded in."""
        dev = wav.device
        basis = self._basis_on(dev)
        head = (ops.P(wav), wav.stride(0), ops.P(ns_dev), N, Lm, ops.P(basis), 1 if self.reflect else 0)
        if self.running:
            ws = torch.empty(query("ds2_spect_running_ws_bytes", N, Lm), dtype=torch.uint8, device=dev)
            tail = (ops.P(None), 0, ops.P(None), 0, ops.P(None), 0, ops.P(None)) if aug is None else \
                (ops.P(aug[0]), aug[1], ops.P(aug[2]), aug[3], ops.P(aug[4]), aug[5], ops.P(aug[6]))
            call("ds2_spectrogram_running", *head, self.running_floor, *self.running_prior, ops.P(out), ops.P(ws),
                 0 if aug is None else 1, *tail, ops.S())
            return
        ws = torch.empty(query("ds2_spect_ws_bytes", N, Lm), dtype=torch.uint8, device=dev)
        head += (1 if self.normalize else 0, ops.P(out), ops.P(ws))
        if aug is None:
            call("ds2_spectrogram", *head, ops.S())
        else:
            call("ds2_spectrogram_aug", *head, ops.P(aug[0]), aug[1], ops.P(aug[2]), aug[3], ops.P(aug[4]), aug[5], ops.P(aug[6]), ops.S())

    def _call_wave_augmented(self, wav, ns, augment, wd=None):
        """__call__ with the waveform augmentations in front: tempo (ds2_wsola), then reverberation (ds2_reverb; it keeps every
        length), then gain / noise (ds2_wave_energy + ds2_wave_mix), then the spectrogram call on the new buffer.  Frame counts, percentages and Tmax follow the lengths after
        the tempo change, which the host knows in closed form (augment.wsola_out_len): nothing is read back.  wd: the WaveDraws
        of these rows when they were drawn already (collate).  wav / ns are the 16 kHz signal: a front-end with input_rate has
        resampled before it comes here."""
        wa, dev, N = self.wave_augment, wav.device, wav.shape[0]
        if wd is None:
            wd = wa.draw(ns.numpy(), self.rng)
        ns2 = torch.from_numpy(wd.nsamples.astype(np.int32))
        Lm = int(ns2.max())
        Tmax = 1 + Lm // HOP
        frames = 1 + ns2.to(torch.int64) // HOP
        sa = self.spec_augment
        sdraws = list(sa.draw(frames.numpy(), N_BIN, self.rng)) if augment else []
        views = self.upload_draws([ns.numpy()] + wd.arrays() + sdraws + wd.rir_arrays(), dev)
        ns_dev, (noise_off, tempo, gain, level, noise_start) = views[0], views[1:6]
        rir_off, rir_len, rir_peak = views[-3:]
        offsets = None
        if tempo is not None:
            wav, ns_dev, offsets = ops.wsola(wav, ns_dev, tempo, Lm, int(wd.segments.max()))
        if rir_off is not None:
            rirs = wa.rir_bank.samples
            if rirs.device != dev:
                raise Ds2HipError("the bank of impulse responses lives on %s, the waveforms on %s" % (rirs.device, dev))
            wav = ops.reverb(wav, ns_dev, rirs, rir_off, rir_len, rir_peak)
        if gain is not None or level is not None:
            bank = wa.noise_bank.samples if level is not None else None
            if bank is not None and bank.device != dev:
                raise Ds2HipError("the noise bank lives on %s, the waveforms on %s" % (bank.device, dev))
            wav = ops.wave_mix(wav, ns_dev, gain, level, bank, noise_off, noise_start)
        self.last_wave = (wd, offsets)
        out = torch.empty((N, 1, N_BIN, Tmax), dtype=torch.float32, device=dev)
        if augment:
            warp, fmask, tmask = views[6:9]
            self.last_coef = torch.empty((N, 3), dtype=torch.float32, device=dev)
            self._launch(wav, ns_dev, N, Lm, out, (warp, sa.W, fmask, sdraws[1].shape[1], tmask, sdraws[2].shape[1], self.last_coef))
        else:
            self._launch(wav, ns_dev, N, Lm, out, None)
        pct = (frames.to(torch.float64) / float(Tmax)).to(torch.float32)
        return out, pct, frames

    def stream(self, capacity, device):
        """A streaming handle over `capacity` slots (``SpectStream``): audio fed in chunks of any lengths gives the frames of this
        front-end's one-shot call on the whole clip, bit for bit.  Needs a causal front-end: zero centre padding and
        normalize="running" or False."""
        return SpectStream(self, capacity, device)

    @staticmethod
    def upload_draws(draws, dev):
        """Host arrays of draws (SpecAugment.draw's (warp_draw, fmask, tmask); WaveDraws.arrays()) -> device views of ONE pinned,
        non-blocking upload (None for None or an array without entries).  The views keep the upload alive.  8-byte arrays are
        placed on 8-byte boundaries."""
        draws = [np.zeros(0, np.int32) if a is None else a for a in draws]
        parts = []
        for a in draws:                                                                   # float32 bits travel as int32 words
            if a.dtype.itemsize == 8 and sum(p.size for p in parts) % 2:
                parts[-1] = np.concatenate([parts[-1], np.zeros(1, np.int32)])
            parts.append(np.ascontiguousarray(a).view(np.int32).reshape(-1))
        host = torch.from_numpy(np.concatenate(parts)).pin_memory()
        buf = host.to(dev, non_blocking=True)
        views, o = [], 0
        for a, p in zip(draws, parts):
            v = buf[o:o + a.size * (a.dtype.itemsize // 4)]
            views.append(v.view(_TORCH_DTYPE[a.dtype]).reshape(a.shape) if a.size else None)
            o += p.size
        return views

    def collate(self, waveforms, transcripts=None, int16_scale=False, augment=False, rates=None):
        """waveforms: list of 1-D float tensors.  Sorts by length descending (as _collate_fn sorts by frame count,
        data_loader.py:251; with wave_augment by the length AFTER the tempo change; with input_rate the resampled length is
        monotone in the given one, so the order is that of the 16 kHz clips), pads, uploads and runs the front-end.
        Returns (inputs, input_percentages, order), or -- with
        `transcripts` (one sequence of label indices per waveform) -- the reference's whole batch tuple
        (inputs, targets, input_percentages, target_sizes) in the sorted order, as _collate_fn builds it (data_loader.py:259-270).

        AMPLITUDE: log1p(|STFT|) is not scale-free.  The reference's load_audio (data_loader.py:23-30) hands
        compute_spectrogram samples in [-1, 1] (int16 / 32767); pass waveforms on that scale, or raw int16-range samples with
        int16_scale=True (they are divided by 32767 here, as load_audio does)."""
        wd = eff = None
        if self.bank is not None:
            # a set of rates and / or speed perturbation: the order is that of the lengths at 16 kHz (after speed and tempo)
            base, wa = self._row_rates(rates, len(waveforms)), self.wave_augment
            lens = [len(w) for w in waveforms]
            if wa is not None and wa.speed_choices:
                wd = wa.draw(lens, self.rng, rates=base)
                eff = wd.rates.tolist()
            else:
                eff = base
                if wa is not None and wa.active:
                    wd = wa.draw([self.bank.out_len(n, r) for n, r in zip(lens, eff)], self.rng)
            key = wd.nsamples if wd is not None else [self.bank.out_len(n, r) for n, r in zip(lens, eff)]
            order = sorted(range(len(waveforms)), key=lambda i: -int(key[i]))
            wd = wd.take(order) if wd is not None else None
        elif rates is not None:
            self._row_rates(rates, len(waveforms))
        elif self.wave_augment is not None and self.wave_augment.active:
            # the reference augments every clip as the sampler hands it out and _collate_fn sorts the RESULTS: draw in the given
            # order, sort by the length after the tempo change (known on the host)
            # (with input_rate: of the 16 kHz signal, the one the augmentations work on)
            rs = self.resampler
            wd = self.wave_augment.draw([len(w) if rs is None else rs.out_len(len(w)) for w in waveforms], self.rng)
            order = sorted(range(len(waveforms)), key=lambda i: -int(wd.nsamples[i]))
            wd = wd.take(order)
        else:
            order = sorted(range(len(waveforms)), key=lambda i: -len(waveforms[i]))
        Lmax = max(len(w) for w in waveforms)
        buf = torch.zeros((len(waveforms), Lmax), dtype=torch.float32)
        for r, i in enumerate(order):
            buf[r, :len(waveforms[i])] = torch.as_tensor(waveforms[i], dtype=torch.float32)
        if int16_scale:
            buf /= 32767.0
        lens = [len(waveforms[i]) for i in order]
        if eff is not None and wd is None:
            inputs, pct, _ = self(buf.cuda(), lens, augment=augment, rates=[eff[i] for i in order])
        elif wd is None:
            inputs, pct, _ = self(buf.cuda(), lens, augment=augment)
        else:
            wav, ns = buf.cuda(), torch.tensor(lens, dtype=torch.int32)
            if eff is not None:
                wav, _, ns = self.bank._run(wav, ns, [eff[i] for i in order])
            if self.resampler is not None:
                wav, _, ns = self.resampler._run(wav, ns)
            inputs, pct, _ = self._call_wave_augmented(wav, ns, augment, wd)
        if transcripts is None:
            return inputs, pct, order
        tg = [torch.as_tensor(transcripts[i], dtype=torch.int64).reshape(-1) for i in order]
        target_sizes = torch.tensor([len(t) for t in tg], dtype=torch.int32)
        targets = torch.cat(tg) if tg else torch.zeros(0, dtype=torch.int64)
        return inputs, targets, pct, target_sizes


SPECT_ROW_WORDS = 8        # int32 words of one ds2_spect_stream_row: slot, src, carried, n_new, frames_before, emit, final, fresh
_ROW_STAGING = ops.PinnedRing()


class SpectStream:
    """The streaming form of a ``SpectrogramFrontEnd`` (csrc/ds2_spect.hip, ds2_spect_stream_feed): per slot the device keeps the
    samples that frames not yet complete need and the running statistics; the host keeps the sample count, from which every count
    of a feed follows in closed form (``plan_wave``), so nothing is read back."""

    def __init__(self, front_end, capacity, device):
        if front_end.reflect:
            raise ValueError("streaming needs pad_mode='constant': reflect padding reads samples that have not arrived")
        if front_end.normalize is True:
            raise ValueError("streaming needs normalize='running' (or False): the mean and the standard deviation of the whole "
                             "utterance are not causal")
        if front_end.wave_augment is not None and front_end.wave_augment.active:
            raise ValueError("streaming takes the audio as it arrives: a front-end with wave_augment cannot be streamed")
        if int(capacity) < 1:
            raise ValueError("capacity must be >= 1, got %s" % (capacity,))
        self.front_end, self.capacity, self.device = front_end, int(capacity), torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        S = self.capacity
        self._state = torch.zeros(query("ds2_spect_stream_state_bytes", S), dtype=torch.uint8, device=self.device)
        self.samples, self.ended, self._fresh = [0] * S, [False] * S, [True] * S
        # a front-end with input_rate: the chunks arrive at that rate and pass a ResampleStream over the same slots first
        # (with a set of rates: a BankStream, each slot at the rate reset() gives it)
        self._resample = front_end.resampler.stream(S, self.device) if front_end.resampler is not None else None
        if front_end.rates is not None:
            self._resample = front_end.bank.stream(S, self.device)

    def reset(self, slots=None, rates=None):
        """These slots (None = all) start a new stream: their carry and statistics read as empty from the next feed on; nothing
        is launched.  rates: with a front-end built with a set of rates, the rate of each slot's new stream (None = the rate it
        had); a slot is fed only once it has one."""
        if rates is not None and self.front_end.rates is None:
            raise ValueError("rates=... belongs to a front-end built with a set of rates (input_rate=(...))")
        slots = list(range(self.capacity)) if slots is None else [int(v) for v in slots]
        for s in slots:
            if not 0 <= s < self.capacity:
                raise ValueError("slot %d is not a slot of this stream (capacity %d)" % (s, self.capacity))
        if rates is not None:                  # refuses a rate that is not of the set before anything is reset
            self._resample.reset(slots, rates)
        elif self._resample is not None:
            self._resample.reset(slots)
        for s in slots:
            self.samples[s], self.ended[s], self._fresh[s] = 0, False, True

    def frames(self, slot):
        """frames emitted so far for the slot's stream"""
        s = int(slot)
        return 1 + self.samples[s] // HOP if self.ended[s] else self.samples[s] // HOP

    def feed(self, slots, wav, nsamples, final=()):
        """wav: [len(slots)][L] float32 on the device, row i = the nsamples[i] >= 0 new samples of slots[i]; final: the slots
        whose utterance ends with this feed.  Returns (spect (len(slots), 1, 161, Tc) float32 with Tc the largest count of new
        frames -- possibly 0 --, frames [len(slots)] ints): row i holds frames[i] new frames, zero beyond them.  With the
        front-end's input_rate the chunks are at that rate; ``samples`` and ``frames`` go on counting the 16 kHz signal."""
        fe, S = self.front_end, self.capacity
        if self._resample is not None:        # the same argument checks, on the same slots: it refuses what this feed would refuse
            slots, final = [int(s) for s in slots], [int(s) for s in final]
            wav, nsamples = self._resample.feed(slots, wav, nsamples, final)
        sl, fin = [int(s) for s in slots], set(int(s) for s in final)
        if not sl or len(set(sl)) != len(sl) or any(not 0 <= s < S for s in sl):
            raise ValueError("slots must be distinct and lie in [0, %d), got %s" % (S, sl))
        if not fin <= set(sl):
            raise ValueError("final names slots that are not in this feed: %s" % sorted(fin - set(sl)))
        ns = [int(v) for v in nsamples]
        if wav.dim() != 2 or wav.shape[0] != len(sl) or len(ns) != len(sl) or any(v < 0 or v > wav.shape[1] for v in ns):
            raise ValueError("expected a [%d][L] waveform chunk and %d sample counts in [0, L], got %s and %s"
                             % (len(sl), len(sl), tuple(wav.shape), ns))
        for s in sl:
            if self.ended[s]:
                raise ValueError("the stream of slot %d has ended (a final feed); reset it first" % s)
        if not wav.is_cuda or wav.device != self.device:
            raise Ds2HipError("SpectStream needs the waveforms on %s; there is no CPU path" % self.device)
        wav = wav.float()
        if wav.shape[1] and wav.stride(1) != 1:
            wav = wav.contiguous()
        plans = [plan_wave(self.samples[s], n, s in fin) for s, n in zip(sl, ns)]
        table = np.array([(s, i, 0 if self._fresh[s] else p.carried, n, p.frames_before, p.emit, int(s in fin), int(self._fresh[s]))
                          for i, (s, n, p) in enumerate(zip(sl, ns, plans))], dtype=np.int32)
        assert all(self.samples[s] == 0 for s in sl if self._fresh[s]) and all(0 <= p.new_carry < N_FFT for p in plans)
        max_new, Tc = max(ns), max(p.emit for p in plans)
        rows = _ROW_STAGING.stage(self.device, [table.reshape(-1)])
        out = torch.empty((len(sl), 1, N_BIN, Tc), dtype=torch.float32, device=self.device)
        ws = torch.empty(query("ds2_spect_stream_ws_bytes", len(sl), max_new, Tc), dtype=torch.uint8, device=self.device)
        call("ds2_spect_stream_feed", ops.P(wav) if max_new else ops.P(None), wav.stride(0) if max_new else 0, ops.P(rows), len(sl),
             max_new, Tc, S, ops.P(fe._basis_on(self.device)), 2 if fe.running else 0, fe.running_floor, *fe.running_prior,
             ops.P(self._state), ops.P(out) if Tc else ops.P(None), ops.P(ws), ops.S())
        for s, n in zip(sl, ns):
            self.samples[s] += n
            self.ended[s], self._fresh[s] = s in fin, False
        return out, [p.emit for p in plans]
