"""SpecAugment as the reference's loader applies it (``augmentation.spec_augment: True`` -> ``spec_augment(spect)``,
loader/spec_augment.py:68-115, called per clip after normalisation, loader/data_loader.py:162-163): the random DRAWS are made here
on the host, everything that touches the spectrogram runs on the device (csrc/ds2_spect.hip).

The reference's time warp is not the paper's: ``time_warp`` (:48-65, always its default W = 5 -- ``time_warping_para`` is never
passed on) picks a frame i, reads the spectrogram VALUE pt = spec[F//2][i] and uses it as a time coordinate of the single control
point (F//2, pt) -> (F//2, pt + d) of ``sparse_image_warp``.  The resulting flow is affine in (f, t), zero along frequency, and
depends on the 3 x 3 block of ``randn / 1e10`` that loader/sparse_image_warp.py:170 puts into the otherwise singular system; so
that block is part of the draw.  This is what models trained with the reference's configurations have seen, and what is
reproduced.

Deviation: a clip with T <= 2W frames (0.1 s) makes the reference's ``randrange(W, T - W)`` raise ValueError; here it is left
unwarped (masks still apply).

``WaveAugment`` covers what the loader does to the SAMPLES before the STFT (loader/data_loader.py:151-159): the tempo / gain
perturbation of ``load_randomly_augmented_audio`` (:392-404, ``augmentation.speed_volume_perturb``) and ``NoiseInjection``
(:97-128, ``augmentation.noise_dir`` / ``noise_prob`` / ``noise_min`` / ``noise_max``).  Again the draws are made here, in the
reference's order, and the samples are touched on the device only (csrc/ds2_waveaug.hip).  The tempo change is the project's own
WSOLA with sox's default ``tempo`` parameters; its length rule is mirrored here (``wsola_out_len``) so that the frame counts of a
batch are known without reading anything back.  Deviations from the reference: no sample parity with sox,
no 16-bit requantisation or dither, a clip longer than its noise recording gets no noise (the reference's assertion fails), a
noise crop without energy adds nothing (the reference produces NaN)."""
import math

import numpy as np

MAX_MASKS = 4           # masks per axis and clip that the kernels take


class SpecAugment:
    def __init__(self, frequency_masking_para=27, time_masking_para=70, frequency_mask_num=1, time_mask_num=1, W=5):
        self.frequency_masking_para, self.time_masking_para = frequency_masking_para, time_masking_para
        self.frequency_mask_num, self.time_mask_num, self.W = int(frequency_mask_num), int(time_mask_num), int(W)
        self._check()

    def _check(self):
        if not (0 <= self.frequency_mask_num <= MAX_MASKS and 0 <= self.time_mask_num <= MAX_MASKS):
            raise ValueError("the device kernels take up to %d frequency and %d time masks per clip; got %d / %d"
                             % (MAX_MASKS, MAX_MASKS, self.frequency_mask_num, self.time_mask_num))
        if self.W < 1:
            raise ValueError("W must be positive")

    def _masks(self, rng, num, para, size):
        m = np.zeros((num, 2), np.int32)
        for k in range(num):
            w = int(rng.uniform(0.0, para))                 # spec_augment.py:99-100 / :108-109
            if size - w < 0:                                # :101 / :110: a mask wider than the axis is skipped
                continue
            m[k] = int(rng.integers(0, size - w, endpoint=True)), w      # random.randint: both ends inclusive
        return m

    def draw(self, frames, n_bins, rng):
        """One set of draws per clip from a numpy.random.Generator, in the reference's order (warp, frequency masks, time masks).
        frames: the clips' frame counts.  Returns (warp_draw [N][12] float32: i, d, the nine values of randn(3, 3) / 1e10, 0;
        fmask [N][MF][2] int32, tmask [N][MT][2] int32: start and width, width 0 = no mask)."""
        self._check()
        frames = np.asarray(frames, np.int64).reshape(-1)
        N, W = len(frames), self.W
        warp = np.zeros((N, 12), np.float32)
        fmask = np.zeros((N, self.frequency_mask_num, 2), np.int32)
        tmask = np.zeros((N, self.time_mask_num, 2), np.int32)
        for n, T in enumerate(frames):
            T = int(T)
            if T > 2 * W:
                warp[n, 0] = rng.integers(W, T - W)         # random.randrange(W, T - W): upper end exclusive (:56)
                warp[n, 1] = rng.integers(-W, W)            # random.randrange(-W, W) (:60)
                warp[n, 2:11] = rng.standard_normal(9) / 1e10
            else:
                warp[n, 0] = -1
            fmask[n] = self._masks(rng, self.frequency_mask_num, self.frequency_masking_para, int(n_bins))
            tmask[n] = self._masks(rng, self.time_mask_num, self.time_masking_para, T)
        return warp, fmask, tmask


# ---- waveform augmentation -------------------------------------------------------------------------------------------------
WSOLA_SEGMENT, WSOLA_SEARCH, WSOLA_OVERLAP = 1312, 234, 192      # sox `tempo` defaults at 16 kHz: 82 ms, 14.68 ms, 12 ms
WSOLA_ADVANCE = WSOLA_SEGMENT - WSOLA_OVERLAP


def wsola_start(k, tempo):
    """nominal first input sample of segment k: floor(k * tempo * 1120) in fp64, tempo an fp32 value."""
    return math.floor(k * float(np.float32(tempo)) * float(WSOLA_ADVANCE))


def wsola_segments(nsamples, tempo):
    """ds2_wsola_segments: the number of k with wsola_start(k) + overlap <= nsamples; 0 = the clip is copied unchanged (shorter
    than segment + search, or a tempo outside [0.1, 10])."""
    L, t = int(nsamples), float(np.float32(tempo))
    if not (L >= WSOLA_SEGMENT + WSOLA_SEARCH and np.float32(0.1) <= np.float32(tempo) <= np.float32(10.0)):
        return 0
    k = int((L - WSOLA_OVERLAP) / (t * float(WSOLA_ADVANCE)))
    while wsola_start(k + 1, t) + WSOLA_OVERLAP <= L:
        k += 1
    while k > 0 and wsola_start(k, t) + WSOLA_OVERLAP > L:
        k -= 1
    return k + 1


def wsola_out_len(nsamples, tempo):
    """ds2_wsola_out_len: (S - 1) * 1120 + min(1312, nsamples - wsola_start(S - 1)); nsamples itself for a copied clip."""
    S = wsola_segments(nsamples, tempo)
    if S == 0:
        return max(int(nsamples), 0)
    return (S - 1) * WSOLA_ADVANCE + min(WSOLA_SEGMENT, int(nsamples) - wsola_start(S - 1, tempo))


def speed_rate(rate, speed):
    """The rate in Hz a clip recorded at `rate` is read at so that it plays `speed` times as fast: rate * speed, evaluated exactly
    (the speed through its decimal string, 1.1 is 11 / 10).  Resampling from there to 16 kHz shortens the clip by `speed` and
    moves pitch and formants with it.  Refuses a product that is not an integer number of Hz."""
    import fractions
    eff = fractions.Fraction(int(rate)) * fractions.Fraction(str(speed))
    if eff.denominator != 1 or eff <= 0:
        raise ValueError("rate %d Hz at speed %s is %s Hz: not a positive integer number of Hz" % (rate, speed, eff))
    return int(eff)


class NoiseBank:
    """The noise recordings of ``augmentation.noise_dir`` as ONE device buffer (fp32, back to back) with their offsets.  Reading
    audio files stays with the caller: hand the decoded mono waveforms (at the front-end's sample rate, on the [-1, 1] scale of
    load_audio) to ``from_waveforms``."""

    def __init__(self, samples, offsets):
        self.samples = samples                                   # device float32 [total]
        self.offsets = np.asarray(offsets, np.int64)             # [R + 1]: recording r = samples[offsets[r]:offsets[r + 1]]

    @classmethod
    def from_waveforms(cls, waveforms, rates=None, device="cuda"):
        """rates: the sample rate in Hz of each recording (None = all at 16 kHz already); recordings at other rates are converted
        to 16 kHz once, here, on `device` in one launch (``resample.ResamplerBank``): offsets and lengths are those of the
        converted recordings."""
        import torch
        if isinstance(rates, (str, torch.device)):        # from_waveforms(waveforms, device), as before there were rates
            rates, device = None, rates
        arrays = [np.ascontiguousarray(np.asarray(w, np.float32).reshape(-1)) for w in waveforms]
        if not arrays or any(a.size == 0 for a in arrays):
            raise ValueError("a noise bank needs at least one recording, and none of them empty")
        if rates is not None and any(int(r) != 16000 for r in rates):
            from .resample import ResamplerBank
            rates = [int(r) for r in rates]
            if len(rates) != len(arrays):
                raise ValueError("rates has %d entries for %d recordings" % (len(rates), len(arrays)))
            buf = torch.zeros((len(arrays), max(a.size for a in arrays)), dtype=torch.float32)
            for i, a in enumerate(arrays):
                buf[i, :a.size] = torch.from_numpy(a)
            out, ns16 = ResamplerBank(sorted(set(rates)))(buf.to(device), [a.size for a in arrays], rates)
            offsets = np.concatenate([[0], np.cumsum(ns16.numpy().astype(np.int64))])
            return cls(torch.cat([out[i, :n] for i, n in enumerate(ns16.tolist())]), offsets)
        offsets = np.concatenate([[0], np.cumsum([a.size for a in arrays])])
        return cls(torch.from_numpy(np.concatenate(arrays)).to(device), offsets)

    def __len__(self):
        return len(self.offsets) - 1

    def length(self, r):
        return int(self.offsets[r + 1] - self.offsets[r])


class RirBank:
    """Room impulse responses as ONE device buffer (fp32, back to back) with their offsets and peak taps: the sibling of
    ``NoiseBank`` for ``WaveAugment(rir_bank=...)``.  Reading audio files stays with the caller: hand the decoded mono responses to
    ``from_waveforms``, or build stand-ins with ``synthetic``.  Per response, on the host in fp64 (``prepare``): the peak p is the
    FIRST arg-max of |h| (the direct path: the reverberated clip stays time-aligned with the dry one), the response is cut to
    max_taps taps in all -- everything up to p is kept, a peak at or beyond max_taps is refused, as is an empty or all-zero
    response --, normalised, and rounded to fp32 once."""

    def __init__(self, samples, offsets, peaks):
        self.samples = samples                                   # device float32 [total]
        self.offsets = np.asarray(offsets, np.int64)             # [R + 1]: response r = samples[offsets[r]:offsets[r + 1]]
        self.peaks = np.asarray(peaks, np.int32)                 # [R]: index of the direct-path tap inside response r

    @staticmethod
    def prepare(h, normalize="energy", max_taps=16384):
        """One response through the bank's rules -> (fp32 taps, peak index).  normalize: "energy" divides by sqrt(sum h^2) (the
        reverberated clip keeps roughly its level), "peak" by |h[p]| (the direct path keeps its level), None leaves the taps."""
        h = np.asarray(h, np.float64).reshape(-1)
        if normalize not in ("energy", "peak", None):
            raise ValueError("normalize must be 'energy', 'peak' or None, got %r" % (normalize,))
        if int(max_taps) < 1:
            raise ValueError("max_taps must be >= 1, got %r" % (max_taps,))
        if h.size == 0 or not np.any(h != 0.0):
            raise ValueError("an impulse response must hold at least one non-zero tap")
        if not np.all(np.isfinite(h)):
            raise ValueError("an impulse response must be finite")
        p = int(np.argmax(np.abs(h)))
        if p >= int(max_taps):
            raise ValueError("the peak of the impulse response lies at tap %d, at or beyond max_taps = %d" % (p, max_taps))
        h = h[:int(max_taps)]
        if normalize == "energy":
            h = h / math.sqrt(float(np.sum(h * h)))
        elif normalize == "peak":
            h = h / abs(float(h[p]))
        return h.astype(np.float32), p

    @classmethod
    def from_waveforms(cls, irs, rates=None, device="cuda", normalize="energy", max_taps=16384):
        """irs: the decoded mono responses; rates: the sample rate in Hz of each (None = all at 16 kHz already); responses at other
        rates are converted to 16 kHz once, here, on `device` in one launch (``resample.ResamplerBank``), exactly as
        ``NoiseBank.from_waveforms`` converts its recordings, and the rules above see the converted taps."""
        import torch
        arrays = [np.asarray(h, np.float64).reshape(-1) for h in irs]
        if not arrays:
            raise ValueError("a bank of impulse responses needs at least one")
        if rates is not None and any(int(r) != 16000 for r in rates):
            from .resample import ResamplerBank
            rates = [int(r) for r in rates]
            if len(rates) != len(arrays):
                raise ValueError("rates has %d entries for %d responses" % (len(rates), len(arrays)))
            if any(a.size == 0 for a in arrays):
                raise ValueError("an impulse response must hold at least one non-zero tap")
            buf = torch.zeros((len(arrays), max(a.size for a in arrays)), dtype=torch.float32)
            for i, a in enumerate(arrays):
                buf[i, :a.size] = torch.from_numpy(a.astype(np.float32))
            out, ns16 = ResamplerBank(sorted(set(rates)))(buf.to(device), [a.size for a in arrays], rates)
            out = out.cpu().numpy()
            arrays = [out[i, :n].astype(np.float64) for i, n in enumerate(ns16.tolist())]
        done = [cls.prepare(a, normalize, max_taps) for a in arrays]
        offsets = np.concatenate([[0], np.cumsum([len(h) for h, _ in done])])
        return cls(torch.from_numpy(np.concatenate([h for h, _ in done])).to(device), offsets, [p for _, p in done])

    @staticmethod
    def synthetic_taps(rt60, rng, drr_db=0.0, sample_rate=16000):
        """The fp64 taps of one stand-in response BEFORE the bank's rules: h[0] = 1, h[k] = a g_k exp(-3 ln10 k / (rt60 sample_rate))
        for 0 < k < ceil(rt60 sample_rate), g_k standard normal from rng, a such that sum_{k > 0} h^2 = 10^(-drr_db / 10)."""
        n = int(math.ceil(float(rt60) * float(sample_rate)))
        if n < 1:
            raise ValueError("rt60 * sample_rate must give at least one tap, got rt60 = %r" % (rt60,))
        h = np.zeros(n, np.float64)
        h[0] = 1.0
        if n > 1:
            k = np.arange(1, n, dtype=np.float64)
            tail = rng.standard_normal(n - 1) * np.exp(-3.0 * math.log(10.0) * k / (float(rt60) * float(sample_rate)))
            e = float(np.sum(tail * tail))
            if e > 0.0:
                h[1:] = tail * math.sqrt(10.0 ** (-float(drr_db) / 10.0) / e)
        return h

    @classmethod
    def synthetic(cls, rt60s, rng, drr_db=0.0, sample_rate=16000, device="cuda", **kw):
        """One stand-in response per reverberation time in rt60s (seconds), for users and tools without a corpus of measured
        responses: exponentially decaying Gaussian NOISE behind a unit direct path (``synthetic_taps``), the tail 60 dB down at
        rt60 and drr_db below the direct path in energy -- not a room model: no early reflections, no frequency-dependent decay.
        The taps then go through ``from_waveforms`` (kw: normalize, max_taps).  With a tail louder than the direct path
        (drr_db < 0) the peak may land inside the tail; the bank's rule decides, as for a measured response."""
        taps = [cls.synthetic_taps(t, rng, drr_db, sample_rate) for t in rt60s]
        return cls.from_waveforms(taps, None if int(sample_rate) == 16000 else [int(sample_rate)] * len(taps), device, **kw)

    def __len__(self):
        return len(self.offsets) - 1

    def length(self, r):
        return int(self.offsets[r + 1] - self.offsets[r])


class WaveDraws:
    """One batch's draws of WaveAugment.  tempo / gain / level [N] float32 (None = that step is off for the batch; gain holds the
    LINEAR factor 10^(dB / 20), gain_db the drawn value), noise_off [N] int64 (-1 = no noise for the clip) and noise_start [N] int32
    with level; nsamples [N] int64 = the sample counts after the tempo change, segments [N] = the clips' WSOLA segment counts.
    With speed_choices: speed [N] float64 = the drawn factors, rates [N] int64 = the rates the clips are read at (rate * speed),
    resampled [N] int64 = the sample counts at 16 kHz after that resampling, in front of the tempo change (None otherwise).
    With a rir_bank: rir_off [N] int64 (-1 = the clip stays dry), rir_len / rir_peak [N] int32 (None otherwise)."""

    def __init__(self, tempo, gain, gain_db, level, noise_off, noise_start, nsamples, segments, speed=None, rates=None, resampled=None,
                 rir_off=None, rir_len=None, rir_peak=None):
        self.tempo, self.gain, self.gain_db, self.level = tempo, gain, gain_db, level
        self.noise_off, self.noise_start, self.nsamples, self.segments = noise_off, noise_start, nsamples, segments
        self.speed, self.rates, self.resampled = speed, rates, resampled
        self.rir_off, self.rir_len, self.rir_peak = rir_off, rir_len, rir_peak

    def take(self, order):
        """the draws of the clips `order`, in that order."""
        pick = lambda a: None if a is None else a[np.asarray(order, np.int64)]      # noqa: E731
        return WaveDraws(*[pick(a) for a in (self.tempo, self.gain, self.gain_db, self.level, self.noise_off, self.noise_start,
                                             self.nsamples, self.segments, self.speed, self.rates, self.resampled,
                                             self.rir_off, self.rir_len, self.rir_peak)])

    def arrays(self):
        """the arrays that go to the device, the 8-byte one first (SpectrogramFrontEnd.upload_draws keeps that order)."""
        return [self.noise_off, self.tempo, self.gain, self.level, self.noise_start]

    def rir_arrays(self):
        """the reverberation's arrays for the same upload, the 8-byte one first (all None without a rir_bank)."""
        return [self.rir_off, self.rir_len, self.rir_peak]


class WaveAugment:
    def __init__(self, speed_volume_perturb=False, tempo_range=(0.85, 1.15), gain_range=(-6, 8), noise_bank=None, noise_prob=0.4,
                 noise_levels=(0.0, 0.5), sample_rate=16000, speed_choices=None, rir_bank=None, rir_prob=0.5):
        """rir_bank: None, or a ``RirBank``: per clip, after the gain draw and in front of the noise draws, binomial(1, rir_prob)
        decides whether the clip is reverberated and, if so, rng.choice(len(rir_bank)) picks its response -- only when the bank is
        set, so every other configuration draws what it drew.  On the device the reverberation sits between tempo and gain.
        speed_choices: None, or the factors of speed perturbation by resampling, (0.9, 1.0, 1.1) in the usual recipe: per clip one
        is drawn uniformly -- the FIRST draw of the clip, and only when this is set, so every other configuration draws what it
        drew -- and the clip is resampled as if recorded at rate * speed Hz (pitch and formants move, unlike the tempo change),
        before tempo, gain and noise, which see the result.  The front-end does the resampling (``speed_rate``)."""
        self.speed_choices = None if speed_choices is None else tuple(speed_choices)
        if self.speed_choices is not None and (not self.speed_choices or any(not float(v) > 0.0 for v in self.speed_choices)):
            raise ValueError("speed_choices must be None or positive factors, got %r" % (speed_choices,))
        self.speed_volume_perturb = bool(speed_volume_perturb)
        self.tempo_range, self.gain_range = tuple(tempo_range), tuple(gain_range)
        self.noise_bank, self.noise_prob, self.noise_levels = noise_bank, float(noise_prob), tuple(noise_levels)
        self.sample_rate = int(sample_rate)
        self.rir_bank, self.rir_prob = rir_bank, float(rir_prob)
        if not 0.1 <= min(self.tempo_range) <= max(self.tempo_range) <= 10.0:
            raise ValueError("tempo_range must lie in [0.1, 10]; got %r" % (self.tempo_range,))

    @classmethod
    def from_config(cls, aug_cfg, noise_bank=None, sample_rate=16000, rir_bank=None):
        """From the reference's AugmentationConfig (configs/train_config.py:25-31; duck typed).  noise_bank: the recordings of
        ``aug_cfg.noise_dir`` as a NoiseBank -- required when noise_dir is set, since no file is read here.  rir_bank: a RirBank
        switches reverberation on, with ``aug_cfg.rir_prob`` when the configuration has one (the reference's has not) or 0.5."""
        if getattr(aug_cfg, "noise_dir", "") and noise_bank is None:
            raise ValueError("augmentation.noise_dir is set: pass its recordings as a NoiseBank (NoiseBank.from_waveforms)")
        return cls(speed_volume_perturb=getattr(aug_cfg, "speed_volume_perturb", False),
                   noise_bank=noise_bank if getattr(aug_cfg, "noise_dir", "") else None,
                   noise_prob=getattr(aug_cfg, "noise_prob", 0.4),
                   noise_levels=(getattr(aug_cfg, "noise_min", 0.0), getattr(aug_cfg, "noise_max", 0.5)), sample_rate=sample_rate,
                   rir_bank=rir_bank, rir_prob=getattr(aug_cfg, "rir_prob", 0.5))

    @property
    def active(self):
        return self.speed_volume_perturb or self.noise_bank is not None or bool(self.speed_choices) or self.rir_bank is not None

    def draw(self, nsamples, rng, rates=None):
        """All draws of a batch on the host, from a numpy.random.Generator or RandomState, per clip in the reference's order:
        tempo and gain (load_randomly_augmented_audio, data_loader.py:398-401; both go to sox as '{:.3f}', :383, so they are rounded
        to three decimals here too), binomial(1, noise_prob) (:157), and for a clip that gets noise the recording (:114), the level
        (:115) and rand() for the start (:121: start = rand * (noise_len - data_len) seconds, truncated to samples here; data_len is
        the length AFTER the tempo change).  A clip longer than its recording gets no noise.  Returns a WaveDraws.
        With a rir_bank, between the gain draw and the noise binomial: binomial(1, rir_prob), and for a clip that came up 1
        rng.choice(len(rir_bank)).
        With speed_choices the clip's first draw is its speed, rng.choice(len(speed_choices)); nsamples then counts the samples
        at `rates` (the rate of each clip, None = 16 kHz), and everything after sees ceil(n 16000 / (rate speed)) samples."""
        ns = np.asarray(nsamples, np.int64).reshape(-1).copy()
        N, bank, sr = len(ns), self.noise_bank, float(self.sample_rate)
        if rates is not None and not self.speed_choices:
            raise ValueError("draw(rates=...) belongs to speed_choices: without them the clips come here at 16 kHz")
        speed = eff = resampled = None
        if self.speed_choices:
            rates = [16000] * N if rates is None else list(rates)
            if len(rates) != N:
                raise ValueError("rates has %d entries for %d clips" % (len(rates), N))
            speed, eff, resampled = np.ones(N, np.float64), np.zeros(N, np.int64), ns
        tempo = np.ones(N, np.float32) if self.speed_volume_perturb else None
        gain_db = np.zeros(N, np.float64) if self.speed_volume_perturb else None
        level = np.zeros(N, np.float32) if bank is not None else None
        noise_off = np.full(N, -1, np.int64) if bank is not None else None
        noise_start = np.zeros(N, np.int32) if bank is not None else None
        rirs = self.rir_bank
        rir_off = np.full(N, -1, np.int64) if rirs is not None else None
        rir_len = np.zeros(N, np.int32) if rirs is not None else None
        rir_peak = np.zeros(N, np.int32) if rirs is not None else None
        out_ns, segments = ns.copy(), np.zeros(N, np.int64)
        for n in range(N):
            if self.speed_choices:
                choice = self.speed_choices[int(rng.choice(len(self.speed_choices)))]
                speed[n], eff[n] = choice, speed_rate(rates[n], choice)
                ns[n] = out_ns[n] = -((-int(ns[n]) * 16000) // int(eff[n]))
            if self.speed_volume_perturb:
                tempo[n] = float("%.3f" % rng.uniform(low=self.tempo_range[0], high=self.tempo_range[1]))
                gain_db[n] = float("%.3f" % rng.uniform(low=self.gain_range[0], high=self.gain_range[1]))
                segments[n], out_ns[n] = wsola_segments(ns[n], tempo[n]), wsola_out_len(ns[n], tempo[n])
            if rirs is not None and rng.binomial(1, self.rir_prob):
                r = int(rng.choice(len(rirs)))
                rir_off[n], rir_len[n], rir_peak[n] = rirs.offsets[r], rirs.length(r), rirs.peaks[r]
            if bank is not None and rng.binomial(1, self.noise_prob):
                r = int(rng.choice(len(bank)))
                lv = rng.uniform(*self.noise_levels)
                u = rng.random()
                noise_len, data_len = bank.length(r), int(out_ns[n])
                if data_len > noise_len:
                    continue
                start = int(u * (noise_len / sr - data_len / sr) * sr)
                level[n], noise_off[n], noise_start[n] = lv, bank.offsets[r], min(max(start, 0), noise_len - data_len)
        gain = np.power(10.0, gain_db / 20.0).astype(np.float32) if gain_db is not None else None
        return WaveDraws(tempo, gain, gain_db, level, noise_off, noise_start, out_ns, segments, speed, eff, resampled,
                         rir_off, rir_len, rir_peak)
