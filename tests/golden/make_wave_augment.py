#!/usr/bin/env python3
"""Generate the waveform-augmentation fixtures tests/golden/waveaug/*.npz from the REAL reference: ``loader/data_loader.py`` imported
unmodified under the stub harness (ref_harness.py) plus stub ``librosa`` / ``sox`` / ``torchaudio`` modules, and its own
``NoiseInjection.inject_noise_sample`` (:118-128) called on in-memory arrays.  Run in the build container only:

    python tests/golden/make_wave_augment.py      # rewrites tests/golden/waveaug/* and prints one line per fixture

``sox.file_info.duration`` and ``audio_with_sox`` (the two places where the reference goes to the sox binary) are replaced by
stand-ins that answer from an in-memory noise array: the duration is len(noise) / 16000, the crop is
noise[round(start * 16000) :][: len(data)].  ``numpy.random.rand`` is pinned for the call so that the crop starts where the fixture
says.  What the fixtures pin is therefore the MIX ARITHMETIC of :125-127 in the reference's own fp32 evaluation -- not sox's crop,
resampling, 16-bit requantisation or dither (README.md says so too).
Every file holds: data (L) f32 = the clip as handed to inject_noise_sample (for a `gain_db` fixture: wave_augment_reference.gain
of `raw`), noise (R) f32 = the whole recording, level, start, out (L) f32 = the reference's output, scale32 = level * rms(data) /
rms(noise crop) evaluated as the reference's fp32 expressions, scale64 = the same in fp64.  Fixtures named hand_* were NOT run
through the reference (it has no "no noise" switch per call, and a silent crop makes it divide by zero): out = data.
It also measures the WSOLA dot-product margin on the tests' inputs (wave_augment_reference.wsola_cases) and writes
reference_noise.json + README.md.  Nothing here is used by the product path."""
import importlib
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import ref_harness  # noqa: E402
import wave_augment_reference as R  # noqa: E402

OUT = os.path.join(HERE, "waveaug")
SR = 16000


def load_reference():
    ref_harness._install_stubs()
    for name in ("librosa", "librosa.display", "librosa.util", "sox", "torchaudio", "matplotlib", "matplotlib.pyplot"):
        if name not in sys.modules:
            try:
                importlib.import_module(name)
            except Exception:
                m = types.ModuleType(name)
                m.use = lambda *a, **k: None                    # matplotlib.use('Agg'), spec_augment.py:42
                m.set_audio_backend = lambda *a, **k: None      # torchaudio.set_audio_backend("sox_io"), data_loader.py:17
                sys.modules[name] = m
    if not hasattr(sys.modules["sox"], "file_info"):
        sys.modules["sox"].file_info = types.SimpleNamespace(duration=None)
    if ref_harness.REFERENCE_ROOT not in sys.path:
        sys.path.insert(0, ref_harness.REFERENCE_ROOT)
    return importlib.import_module("deepspeech_pytorch.loader.data_loader")


def reference_mix(dl, data, noise, level, start):
    """inject_noise_sample on a copy of data, with the two sox calls answered from `noise`."""
    recordings = {"bank.wav": noise}
    dl.sox.file_info.duration = lambda path: len(recordings[path]) / SR
    seen = {}

    def crop(path, sample_rate, start_time, end_time):
        s = int(round(start_time * sample_rate))
        seen["start"] = s
        return recordings[path][s:s + len(data)].copy()

    dl.audio_with_sox = crop
    inj = dl.NoiseInjection.__new__(dl.NoiseInjection)           # __init__ only lists the files of a directory
    inj.sample_rate, inj.noise_levels, inj.paths = SR, (0, 0.5), ["bank.wav"]
    room = len(noise) - len(data)
    rand = np.random.rand
    np.random.rand = lambda: (start / room if room else 0.0)
    try:
        out = inj.inject_noise_sample(data.copy(), "bank.wav", level)
    finally:
        np.random.rand = rand
    assert seen["start"] == start, (seen, start)
    assert out.dtype == np.float32
    return out


def clip(L, seed, amp=0.3):
    rs = np.random.RandomState(seed)
    t = np.arange(L) / SR
    return (amp * np.sin(2 * np.pi * 440.0 * t + rs.uniform(0, 6)) + 0.1 * amp * rs.standard_normal(L)).astype(np.float32)


# (name, L, noise length, start (None = noise_len - L), level, gain_db or None); every clip <= 4000 samples.  2048 = the samples one
# sweep of the energy kernel's eight workgroups covers (its partial-sum split); 256 = one workgroup's share of a sweep.
CASES = [("len1", 1, 50, 7, 0.4, None), ("len255", 255, 700, 100, 0.25, None), ("len256", 256, 700, 0, 0.5, None),
         ("len257", 257, 700, None, 0.1, None), ("len2047", 2047, 3000, 900, 0.3, None), ("len2048", 2048, 3000, None, 0.45, None),
         ("len2049", 2049, 2049, 0, 0.2, None), ("len3999", 3999, 4000, 1, 0.35, None), ("gain_clamps", 1500, 2500, 321, 0.3, 14.0)]


def main():
    os.makedirs(OUT, exist_ok=True)
    dl = load_reference()
    fig = {}
    for k, (name, L, R_len, start, level, gain_db) in enumerate(CASES):
        raw = clip(L, 100 + k)
        data = R.gain(raw, gain_db) if gain_db is not None else raw
        noise = (0.2 * np.random.RandomState(200 + k).standard_normal(R_len)).astype(np.float32)
        start = R_len - L if start is None else start
        out = reference_mix(dl, data, noise, level, start)
        crop = noise[start:start + L]
        ne32 = np.sqrt(crop.dot(crop) / crop.size)               # data_loader.py:125-126, as written there
        de32 = np.sqrt(data.dot(data) / data.size)
        scale32 = np.float32(np.float32(level) * de32 / ne32)
        scale64 = R.scale(data, crop, level)
        extra = {"raw": raw, "gain_db": np.float64(gain_db)} if gain_db is not None else {}
        if gain_db is not None:
            assert np.abs(data).max() == 1.0 and (np.abs(data) == 1.0).sum() > 10          # the gain does clamp
        np.savez_compressed(os.path.join(OUT, name + ".npz"), data=data, noise=noise, level=np.float64(level), start=np.int64(start),
                            out=out, scale32=scale32, scale64=np.float64(scale64), **extra)
        fig[name] = float(np.abs(R.mix(data, crop, level) - out).max())
        print("%-12s L %4d noise %4d start %4d level %.2f scale32 %.8g scale64 %.17g  max |f64 - reference| %.3e"
              % (name, L, R_len, start, level, scale32, scale64, fig[name]))
    # not run through the reference: no noise for the clip, and a noise crop without energy
    for name, L, level, noise in (("hand_no_noise", 300, 0.0, np.zeros(0, np.float32)),
                                  ("hand_silent_crop", 513, 0.3, np.zeros(600, np.float32))):
        data = clip(L, 300 + L)
        np.savez_compressed(os.path.join(OUT, name + ".npz"), data=data, noise=noise, level=np.float64(level), start=np.int64(0),
                            out=data, scale32=np.float32(0), scale64=np.float64(0))
        fig[name] = 0.0
    # WSOLA: the largest |fp32 dot - fp64 dot| that numpy's own fp32 evaluation shows on the tests' inputs, along the fp64 path
    worst = 0.0
    for name, x, tempo, _ in R.wsola_cases():
        _, chosen = R.wsola(x, tempo)
        prev = 0
        for k in range(1, len(chosen)):
            worst = max(worst, float(np.abs(R.dots(x, prev, k, tempo, np.float32).astype(np.float64) - R.dots(x, prev, k, tempo)).max()))
            prev = R.start(k, tempo) + int(chosen[k])
    fig["wsola_dot_fp32_error"] = worst
    fig["wsola_dot_margin"] = 4 * worst
    print("wsola: max |fp32 dot - fp64 dot| %.3e -> margin %.3e" % (worst, 4 * worst))
    with open(os.path.join(OUT, "reference_noise.json"), "w") as f:
        json.dump(fig, f, indent=1, sort_keys=True)
        f.write("\n")
    with open(os.path.join(OUT, "README.md"), "w") as f:
        f.write("# Waveform-augmentation fixtures\n\nWritten by `tests/golden/make_wave_augment.py` (see its docstring for the contents "
                "of a file) from the reference's own `NoiseInjection.inject_noise_sample`, with `sox.file_info.duration` and "
                "`audio_with_sox` answered from an in-memory noise array.\n\n**Pinned:** the mix arithmetic of "
                "`data_loader.py:125-127` (`data += noise_level * noise * rms(data) / rms(noise)`) in the reference's own fp32 "
                "evaluation.  **Not pinned:** anything sox does -- the crop position to the sample, resampling, the 16-bit "
                "requantisation and dither of its output file, and the whole `tempo` / `gain` effect chain (sox is not installed "
                "where these fixtures are made).  `hand_*` fixtures were not run through the reference: it has no per-call "
                "\"no noise\" switch, and a noise crop without energy makes it divide by zero; there `out = data`.\n\n"
                "`reference_noise.json` and the table hold, per fixture, max |fp64 restatement - reference output| with the "
                "restatement of `tests/wave_augment_reference.py`: the fp32 noise of the reference itself and the yardstick of "
                "`tests/test_gpu_wave_augment.py`.\n\n| fixture | samples | max abs difference |\n|---|---|---|\n")
        for name in sorted(n for n in fig if not n.startswith("wsola")):
            f.write("| %s | %d | %.3e |\n" % (name, len(np.load(os.path.join(OUT, name + ".npz"))["data"]), fig[name]))
        f.write("\n## WSOLA dot-product margin\n\nOn the inputs of `wave_augment_reference.wsola_cases()`, along the offsets the fp64 "
                "restatement chooses, the largest |fp32 dot product - fp64 dot product| over all segments and candidate offsets, "
                "with the fp32 one evaluated by numpy (`numpy.dot` on float32 arrays): **%.3e**.  The tests allow a reported "
                "offset's fp64 dot product to lie below its segment's fp64 maximum by 4 x that = **%.3e** "
                "(`wsola_dot_margin` in `reference_noise.json`).\n" % (worst, 4 * worst))


if __name__ == "__main__":
    main()
