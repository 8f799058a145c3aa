"""Device-side replacement for the CPU spectrogram workers of the reference loader: ``SpectrogramParser.compute_spectrogram``
(loader/data_loader.py:73-94) for every utterance of a batch + the zero-padded batch layout of ``_collate_fn`` (:247-270), as one
call on the HIP kernels of csrc/ds2_spect.hip.  Output = exactly the ``inputs`` / ``input_percentages`` the model's
``training_step`` takes.  Geometry: 16 kHz, 20 ms window, 10 ms stride (n_fft 320, hop 160 -> 161 bins), the geometry this
front-end's DFT GEMM is specialised for (the conv kernels take any bin count, ``ops.conv_rows``; 8 kHz / 81-bin spectrograms have
to come from elsewhere); the window type follows ``SpectConfig.window`` (enums.py:8-14).  With ``augment=True`` the reference's
``spec_augment`` (loader/spec_augment.py:68-115, see ``augment.SpecAugment``) is folded into the same call.  A front-end built with
``wave_augment=augment.WaveAugment(...)`` first runs the loader's waveform augmentations (tempo, gain, noise injection,
data_loader.py:151-159) on the device, so one call covers everything ``parse_audio`` does.

The reference's STFT lives in a third-party dependency that is not vendored and not pinned (``librosa``, requirements.txt:4):
``center=True`` padding is zeros in librosa >= 0.10 (``pad_mode="constant"``, the default here) and reflection before
(``pad_mode="reflect"`` = ``np.pad(y, 160, "reflect")`` for every length >= 1: a clip shorter than the pad is folded as often as
it takes, a single sample repeats)."""
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


class SpectrogramFrontEnd:
    def __init__(self, spect_cfg=None, normalize=True, pad_mode="constant", spec_augment=None, rng=None, wave_augment=None):
        """spec_augment: an ``augment.SpecAugment`` (None = its defaults) used by calls with ``augment=True``; rng: the
        numpy.random.Generator its draws come from (None = a fresh default_rng()).  wave_augment: an ``augment.WaveAugment``
        (None = none) applied to the waveforms of EVERY call, as the reference's loader applies tempo / gain / noise whenever its
        configuration asks for them; its draws come from rng too, before those of SpecAugment."""
        sr = getattr(spect_cfg, "sample_rate", 16000)
        n_fft = int(sr * getattr(spect_cfg, "window_size", 0.02))
        hop = int(sr * getattr(spect_cfg, "window_stride", 0.01))
        if (n_fft, hop) != (N_FFT, HOP):
            raise ValueError("the gfx950 front-end is specialised for n_fft 320 / hop 160 (16 kHz, 20 ms, 10 ms); got %d / %d" % (n_fft, hop))
        if pad_mode not in ("constant", "reflect"):
            raise ValueError("pad_mode must be 'constant' (librosa >= 0.10) or 'reflect'")
        self.window = getattr(spect_cfg, "window", "hamming")
        self.normalize, self.reflect = bool(normalize), pad_mode == "reflect"
        self.spec_augment = spec_augment if spec_augment is not None else SpecAugment()
        self.rng = rng if rng is not None else np.random.default_rng()
        self._basis = {}
        self.last_coef = None            # device [N][3]: the time-warp flow coefficients of the latest augmented call
        self.wave_augment = wave_augment
        self.last_wave = None            # (WaveDraws, device [N][Smax] WSOLA offsets or None) of the latest call with wave_augment

    def _basis_on(self, dev):
        b = self._basis.get(dev)
        if b is None:
            b = self._basis[dev] = torch.from_numpy(dft_basis(self.window)).to(dev)
        return b

    def __call__(self, wav, nsamples, augment=False):
        """wav: [N][Lmax] float32 on a HIP device (row n = utterance n, zero beyond nsamples[n]); nsamples: [N] ints.
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
        if self.wave_augment is not None and self.wave_augment.active:
            return self._call_wave_augmented(wav, ns, augment)
        Tmax = 1 + Lm // HOP
        out = torch.empty((N, 1, N_BIN, Tmax), dtype=torch.float32, device=wav.device)
        ws = torch.empty(query("ds2_spect_ws_bytes", N, Lm), dtype=torch.uint8, device=wav.device)
        basis = self._basis_on(wav.device)
        ns_dev = ns.to(wav.device)       # held in a local until the launch is enqueued (a temporary would be freed -- and its block
        #                                  possibly re-used by the basis upload -- before the kernels read it)
        frames = 1 + ns.to(torch.int64) // HOP
        if augment:
            sa = self.spec_augment
            draws = sa.draw(frames.numpy(), N_BIN, self.rng)
            warp, fmask, tmask = self.upload_draws(draws, wav.device)
            self.last_coef = torch.empty((N, 3), dtype=torch.float32, device=wav.device)
            call("ds2_spectrogram_aug", ops.P(wav), wav.stride(0), ops.P(ns_dev), N, Lm, ops.P(basis),
                 1 if self.reflect else 0, 1 if self.normalize else 0, ops.P(out), ops.P(ws), ops.P(warp), sa.W,
                 ops.P(fmask), draws[1].shape[1], ops.P(tmask), draws[2].shape[1], ops.P(self.last_coef), ops.S())
        else:
            call("ds2_spectrogram", ops.P(wav), wav.stride(0), ops.P(ns_dev), N, Lm, ops.P(basis),
                 1 if self.reflect else 0, 1 if self.normalize else 0, ops.P(out), ops.P(ws), ops.S())
        pct = (frames.to(torch.float64) / float(Tmax)).to(torch.float32)      # _collate_fn: seq_length / float(max_seqlength)
        return out, pct, frames

    def _call_wave_augmented(self, wav, ns, augment, wd=None):
        """__call__ with the waveform augmentations in front: tempo (ds2_wsola), then gain / noise (ds2_wave_energy +
        ds2_wave_mix), then the spectrogram call on the new buffer.  Frame counts, percentages and Tmax follow the lengths after
        the tempo change, which the host knows in closed form (augment.wsola_out_len): nothing is read back.  wd: the WaveDraws
        of these rows when they were drawn already (collate)."""
        wa, dev, N = self.wave_augment, wav.device, wav.shape[0]
        if wd is None:
            wd = wa.draw(ns.numpy(), self.rng)
        ns2 = torch.from_numpy(wd.nsamples.astype(np.int32))
        Lm = int(ns2.max())
        Tmax = 1 + Lm // HOP
        frames = 1 + ns2.to(torch.int64) // HOP
        sa = self.spec_augment
        sdraws = list(sa.draw(frames.numpy(), N_BIN, self.rng)) if augment else []
        views = self.upload_draws([ns.numpy()] + wd.arrays() + sdraws, dev)
        ns_dev, (noise_off, tempo, gain, level, noise_start) = views[0], views[1:6]
        offsets = None
        if tempo is not None:
            wav, ns_dev, offsets = ops.wsola(wav, ns_dev, tempo, Lm, int(wd.segments.max()))
        if gain is not None or level is not None:
            bank = wa.noise_bank.samples if level is not None else None
            if bank is not None and bank.device != dev:
                raise Ds2HipError("the noise bank lives on %s, the waveforms on %s" % (bank.device, dev))
            wav = ops.wave_mix(wav, ns_dev, gain, level, bank, noise_off, noise_start)
        self.last_wave = (wd, offsets)
        out = torch.empty((N, 1, N_BIN, Tmax), dtype=torch.float32, device=dev)
        ws = torch.empty(query("ds2_spect_ws_bytes", N, Lm), dtype=torch.uint8, device=dev)
        basis = self._basis_on(dev)
        head = (ops.P(wav), wav.stride(0), ops.P(ns_dev), N, Lm, ops.P(basis), 1 if self.reflect else 0, 1 if self.normalize else 0,
                ops.P(out), ops.P(ws))
        if augment:
            warp, fmask, tmask = views[6:]
            self.last_coef = torch.empty((N, 3), dtype=torch.float32, device=dev)
            call("ds2_spectrogram_aug", *head, ops.P(warp), sa.W, ops.P(fmask), sdraws[1].shape[1], ops.P(tmask), sdraws[2].shape[1],
                 ops.P(self.last_coef), ops.S())
        else:
            call("ds2_spectrogram", *head, ops.S())
        pct = (frames.to(torch.float64) / float(Tmax)).to(torch.float32)
        return out, pct, frames

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

    def collate(self, waveforms, transcripts=None, int16_scale=False, augment=False):
        """waveforms: list of 1-D float tensors.  Sorts by length descending (as _collate_fn sorts by frame count,
        data_loader.py:251; with wave_augment by the length AFTER the tempo change), pads, uploads and runs the front-end.
        Returns (inputs, input_percentages, order), or -- with
        `transcripts` (one sequence of label indices per waveform) -- the reference's whole batch tuple
        (inputs, targets, input_percentages, target_sizes) in the sorted order, as _collate_fn builds it (data_loader.py:259-270).

        AMPLITUDE: log1p(|STFT|) is not scale-free.  The reference's load_audio (data_loader.py:23-30) hands
        compute_spectrogram samples in [-1, 1] (int16 / 32767); pass waveforms on that scale, or raw int16-range samples with
        int16_scale=True (they are divided by 32767 here, as load_audio does)."""
        wd = None
        if self.wave_augment is not None and self.wave_augment.active:
            # the reference augments every clip as the sampler hands it out and _collate_fn sorts the RESULTS: draw in the given
            # order, sort by the length after the tempo change (known on the host)
            wd = self.wave_augment.draw([len(w) for w in waveforms], self.rng)
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
        if wd is None:
            inputs, pct, _ = self(buf.cuda(), lens, augment=augment)
        else:
            inputs, pct, _ = self._call_wave_augmented(buf.cuda(), torch.tensor(lens, dtype=torch.int32), augment, wd)
        if transcripts is None:
            return inputs, pct, order
        tg = [torch.as_tensor(transcripts[i], dtype=torch.int64).reshape(-1) for i in order]
        target_sizes = torch.tensor([len(t) for t in tg], dtype=torch.int32)
        targets = torch.cat(tg) if tg else torch.zeros(0, dtype=torch.int64)
        return inputs, targets, pct, target_sizes
