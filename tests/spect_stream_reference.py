"""Restatements in numpy fp64 of the running (causal) normalisation of the spectrogram front-end and of the sample plan of its
streaming form, written from the definitions and not from the kernels.

Running normalisation of raw log-magnitudes v [161][T]: frame t is normalised with the mean and the unbiased standard deviation
of ALL values of frames 0..t (plus the prior's pseudo-counts), the standard deviation bounded below by `floor`.

Sample plan: the clip is centre-padded with 160 zeros on both sides, frame t covers padded positions [160 t, 160 t + 320).  A
frame is complete when its last sample has arrived, or when the utterance has ended (then the right padding exists).

SpecAugment on top (tests/spec_augment_reference.py, unchanged, does the warp and the masks): the warp interpolates between two
frames that are each normalised with their own statistics, and its control value is the normalised centre bin of frame i --
which is the plain warp applied to the running-normalised spectrogram."""
import numpy as np

import spec_augment_reference as R

HOP, NFFT, NBIN = 160, 320, 161


def running_stats(v, floor=1e-5, prior=None):
    """(mean [T], rstd [T]) in fp64.  prior: (mean, std, frames) pseudo-counts or None."""
    v = np.asarray(v, np.float64)
    F, T = v.shape
    pm, ps, pf = (0.0, 0.0, 0.0) if prior is None else [float(x) for x in prior]
    cnt0 = F * pf
    S = pm * cnt0 + np.cumsum(v.sum(0))
    Q = (ps * ps + pm * pm) * cnt0 + np.cumsum((v * v).sum(0))
    cnt = F * np.arange(1, T + 1, dtype=np.float64) + cnt0
    mean = S / cnt
    var = np.maximum((Q - cnt * mean * mean) / (cnt - 1.0), 0.0)
    return mean, 1.0 / np.maximum(np.sqrt(var), floor)


def running_normalize(v, floor=1e-5, prior=None):
    mean, rstd = running_stats(v, floor, prior)
    return (np.asarray(v, np.float64) - mean[None, :]) * rstd[None, :]


def spec_augment_running(v, coef, fmask, tmask, floor=1e-5, prior=None):
    """the reference's warp and masks on the running-normalised spectrogram"""
    return R.spec_augment(running_normalize(v, floor, prior), coef, fmask, tmask)


# ---- the sample plan ----------------------------------------------------------------------------------------------------------
def frames_complete(G, ended):
    """frames of a stream whose every sample is known after G samples: frame t needs padded positions < 160 t + 320, and
    160 + G of them exist (320 + G once the utterance has ended)."""
    have = HOP + G + (HOP if ended else 0)
    return max((have - NFFT) // HOP + 1, 0) if have >= NFFT else 0


def sample_plan(G0, n, final):
    """(frames before, frames emitted, window samples in front of the new ones, window length, samples carried on, clip position
    of the window's first sample) by counting positions of the padded clip."""
    f0, f1 = frames_complete(G0, False), frames_complete(G0 + n, final)
    start = HOP * f0                                   # padded position of the first sample a later frame still needs
    have_before, have_after = HOP + G0, HOP + G0 + n + (HOP if final else 0)
    return f0, f1 - f0, have_before - start, have_after - start, 0 if final else have_after - HOP * f1, start - HOP


def padded(x):
    return np.concatenate([np.zeros(HOP), np.asarray(x, np.float64), np.zeros(HOP)])


def feeds_of(L, chunk, final_with_samples=True, empties=True):
    """A clip of L samples cut into feeds of `chunk` samples (None = the whole clip), an empty feed in front of every third one
    when `empties`; the last feed is final and carries the rest, or -- final_with_samples=False -- every sample goes in a feed
    that is not final and a flush-only final feed of 0 samples follows.  Returns [(n_new, final)]."""
    c = L if chunk is None else chunk
    sizes, pos = [], 0
    while L - pos > c:
        sizes.append(c)
        pos += c
    sizes.append(L - pos)
    out = []
    for k, s in enumerate(sizes):
        if empties and k % 3 == 0:
            out.append((0, False))
        last = k == len(sizes) - 1
        out.append((s, last and final_with_samples))
    if not final_with_samples:
        out.append((0, True))
    return out
