"""The waveforms of the spectrogram front-end's edge tests, the fp64 oracle call they are judged by, and an fp32 numpy
restatement of the device pipeline.  Shared by tests/test_gpu_spect.py (device against oracle, bound 2e-4) and
tests/test_spect_fp32_emulation.py (restatement against oracle: every case the device is judged on has to stay within 2e-5
there, a tenth of the device's bound)."""
import numpy as np

from oracle import ds2_oracle as O

HOP, NBIN = 160, 161

# T:       129    128    127    65     64     64     63    3    2    2    1   1
SEAMS = [20480, 20320, 20319, 10240, 10239, 10080, 10079, 320, 319, 160, 159, 2]
FRAME_BATCHES = {"Tmax129": SEAMS, "Tmax1": [159, 2], "Tmax2": [319, 160, 159], "Tmax64": [10239, 10080, 10079, 2],
                 "Tmax65": [10240, 10239, 319]}
REFLECT_LENGTHS = [1, 2, 41, 80, 81, 159, 160, 161]
CLIPS = [10240, 10239, 400]                                        # T = 65, 64, 3
WINDOWS = ["hann", "blackman", "bartlett"]
SIGNAL_KINDS = ["near_silent", "full_scale", "dc", "tone", "int16"]


def noise(seed, L, amp=0.3):
    return (np.random.RandomState(seed).standard_normal(L) * amp).astype(np.float32)


def signal(kind, seed, L):
    g = np.random.RandomState(seed).standard_normal(L)
    if kind == "near_silent":
        y = g * 1e-4
    elif kind == "full_scale":
        y = np.clip(g * 0.5, -1.0, 1.0)
    elif kind == "dc":
        y = g * 0.05 + 0.5
    elif kind == "tone":
        y = 0.4 * np.sin(2 * np.pi * 1000.0 * np.arange(L) / 16000.0) + 1e-3 * g
    elif kind == "int16":
        y = np.round(3000.0 * g) / 32767.0
    else:
        raise ValueError(kind)
    return y.astype(np.float32)


def frame_edge_wavs(batch, normalize):
    """The unnormalised runs carry a one-sample clip too: zero-padded it is an impulse, whose spectrum is flat, so that it has no
    standard deviation to normalise by."""
    lens = FRAME_BATCHES[batch] + ([] if normalize else [1])
    return [noise(100 + k, n) + np.float32(0.01) for k, n in enumerate(lens)]


def reflect_wavs(L):
    return [noise(L, L)]


def window_wavs():
    return [noise(200 + k, n) for k, n in enumerate(CLIPS)]


def signal_wavs(kind):
    return [signal(kind, 300 + k, n) for k, n in enumerate(CLIPS)]


def silent_wavs():
    return [noise(400, CLIPS[0]), np.zeros(CLIPS[1], np.float32), noise(401, CLIPS[2])]


def n65_wavs():
    lens = [160 + 7 * k for k in range(65)]
    assert len(set(lens)) == 65 and {1 + n // HOP for n in lens} == {2, 3, 4}
    return [noise(700 + k, n, 0.05 + 0.005 * k) for k, n in enumerate(lens)]


def n1_wavs():
    return [noise(800, 480)]


def long_wavs():
    return [noise(1000, 480000, 0.1)]


def oracle(w, pad_mode, normalize, window="hamming"):
    with np.errstate(invalid="ignore", divide="ignore"):          # an all-zero clip normalises to 0 / 0
        return O.log_spectrogram(np.asarray(w, np.float64), window=window, normalize=normalize, pad_mode=pad_mode)


def emulate_fp32(w, pad_mode, normalize, window="hamming"):
    """The device pipeline for one clip in numpy float32: float32 DFT basis and matmul over the centre-padded frames, fp32
    log1p(sqrt(re^2 + im^2)), fp64 sum and sum of squares -> fp32 mean and 1 / std, fp32 normalise.  [161][T] float32."""
    from deepspeech.pytorch_amd.spectrogram import dft_basis
    w = np.asarray(w, np.float32)
    yp = np.pad(w, HOP, mode="reflect" if pad_mode == "reflect" else "constant")
    T = 1 + len(w) // HOP
    frames = np.stack([yp[t * HOP:t * HOP + 2 * HOP] for t in range(T)], 0)
    C = frames @ dft_basis(window).T
    re, im = C[:, :NBIN], C[:, NBIN:]
    v = np.log1p(np.sqrt(re * re + im * im)).astype(np.float32)
    if normalize:
        d = v.astype(np.float64)
        mean = d.sum() / d.size
        var = max(((d * d).sum() - d.size * mean * mean) / (d.size - 1.0), 0.0)
        with np.errstate(invalid="ignore", divide="ignore"):
            v = (v - np.float32(mean)) * np.float32(1.0 / np.sqrt(var))
    return v.T
