"""Admission of the cases of tests/test_gpu_spect.py: the device is held to max |device - oracle| < 2e-4 on a case only if an
fp32 numpy restatement of its pipeline (spect_cases.emulate_fp32) stays within 2e-5 of the fp64 oracle on the same waveforms, so
that the bound leaves the MFMA path at least 10x of what plain fp32 arithmetic needs.  Runs without a GPU."""
import numpy as np
import pytest

import spect_cases as S

ADMIT = 2e-5


def admit(label, wavs, pad_mode="constant", normalize=True, window="hamming", nonfinite_ok=()):
    worst = 0.0
    for i, w in enumerate(wavs):
        ref = S.oracle(w, pad_mode, normalize, window)
        emu = S.emulate_fp32(w, pad_mode, normalize, window).astype(np.float64)
        assert emu.shape == ref.shape == (S.NBIN, 1 + len(w) // S.HOP)
        if i in nonfinite_ok:
            assert not np.isfinite(ref).any() and not np.isfinite(emu).any()
            continue
        assert np.isfinite(ref).all() and np.isfinite(emu).all(), (label, len(w))
        err = float(np.abs(emu - ref).max())
        assert err <= ADMIT, (label, len(w), err)
        worst = max(worst, err)
    print("%s [%s, %s, %s]: max |fp32 restatement - oracle| = %.3e" % (label, pad_mode, "normalised" if normalize else "raw", window, worst))


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("pad_mode", ["constant", "reflect"])
@pytest.mark.parametrize("batch", sorted(S.FRAME_BATCHES))
def test_frame_count_edges_are_admitted(batch, pad_mode, normalize):
    admit(batch, S.frame_edge_wavs(batch, normalize), pad_mode, normalize)


@pytest.mark.parametrize("L", S.REFLECT_LENGTHS)
def test_short_reflect_clips_are_admitted(L):
    admit("reflect L=%d" % L, S.reflect_wavs(L), "reflect", False)


@pytest.mark.parametrize("window", S.WINDOWS)
def test_windows_are_admitted(window):
    admit("window", S.window_wavs(), "constant", True, window)


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("kind", S.SIGNAL_KINDS)
def test_signal_classes_are_admitted(kind, normalize):
    admit(kind, S.signal_wavs(kind), "constant", normalize)


@pytest.mark.parametrize("normalize", [True, False])
def test_neighbours_of_a_silent_clip_are_admitted(normalize):
    admit("silent", S.silent_wavs(), "constant", normalize, nonfinite_ok={1} if normalize else ())


def test_batch_size_and_long_clips_are_admitted():
    admit("N=65", S.n65_wavs())
    admit("N=1", S.n1_wavs())
    admit("L=480000", S.long_wavs())
